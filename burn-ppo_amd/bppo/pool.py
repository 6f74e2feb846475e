"""Historical opponent pool (opponent_pool.rs) and the pool training loop (main.rs:729-803).

OpponentPool restates the reference's host bookkeeping: per-checkpoint win-rate and
Swiss-point EMAs updated once per rotation, `(1 - win_rate)^p` sampling of the opponents
all envs share, best-checkpoint and pool-performance metrics, `opponent_stats.json`.
Checkpoints live in memory here (parameters + optional observation normaliser); a run
directory's checkpoints come in through bppo.checkpoint's loaders and add_checkpoint.

The device plays the games: the finished games' seats and placements, and the sums of
queue_game_result per device model slot, come back through bppo_opponents_completions /
bppo_opponents_results (Context.opponent_completions / opponent_results).  PoolTrainer
keeps the device's model slots (at most 15) equal to the pool members in use and runs
one training iteration per step.  One context only: at W > 1 each rank keeps its own sums.

RatingHistory (rating_history.rs:78-341 without the files) keeps every rated game of a run in
a device rating table (bppo.ratings) and refits it on demand; PoolTrainer(rating_history=...)
feeds it each rollout's finished games without taking them through the host.
"""
import json
import os
from dataclasses import asdict, dataclass

import numpy as np

from .checkpoint import to_json_pretty
from .host import schedule_get
from .ppo import Trainer, train_step
from .ratings import PlackettLuceConfig, RatingTable
from .rng import StdRng

MAX_DEVICE_MODELS = 15


@dataclass
class OpponentStats:
    """opponent_pool.rs:32-61, the fields of one `opponents` entry of opponent_stats.json"""
    checkpoint_name: str
    checkpoint_step: int
    win_rate: float = 0.5            # the learner's win rate against it (EMA); 0.5 = neutral
    avg_swiss_points: float = 0.0    # the learner's Swiss points against it (EMA)
    games_played: int = 0


class OpponentPool:
    """opponent_pool.rs:129-963 without the model loading: `available[i]` = OpponentStats,
    `models[i]` = (params, normalizer or None)."""

    def __init__(self, num_players, alpha, exponent, seed):
        self.available = []
        self.models = []
        self.num_opponent_slots = max(int(num_players) - 1, 0)
        self.opponent_select_alpha = float(alpha)
        self.opponent_select_exponent = float(exponent)
        self.rng = StdRng.seed_from_u64(seed)
        self.current_opponents = []
        self.pending_rotation_stats = {}     # pool index -> [wins, games, total Swiss points]

    # -- membership (opponent_pool.rs:248-262, 407-427) --------------------
    def num_available(self):
        return len(self.available)

    def has_opponents(self):
        return bool(self.available)

    def add_checkpoint(self, name, step, params, normalizer=None):
        """a newly saved checkpoint joins the pool with win_rate 0.5; a name already in the
        pool is left alone (an entry that load_opponent_stats made receives its model)"""
        params = np.array(params, np.float32).reshape(-1)
        for i, s in enumerate(self.available):
            if s.checkpoint_name == name:
                if self.models[i] is None:
                    self.models[i] = (params, normalizer)
                return
        self.available.append(OpponentStats(name, int(step)))
        self.models.append((params, normalizer))

    def get_checkpoint_name(self, pool_index):
        if 0 <= pool_index < len(self.available):
            return self.available[pool_index].checkpoint_name
        return f"unknown_{pool_index}"

    # -- sampling (opponent_pool.rs:228-246, 429-490) ----------------------
    def _weight(self, win_rate):
        return (1.0 - win_rate) ** self.opponent_select_exponent

    def sample_opponent(self, exclude=()):
        if not self.available:
            return None
        eligible = [i for i in range(len(self.available)) if i not in exclude]
        if not eligible:                                    # all excluded: any opponent
            return self.rng.gen_range(len(self.available))
        weights = [self._weight(self.available[i].win_rate) for i in eligible]
        total = 0.0
        for w in weights:
            total += w
        if total == 0.0:                                    # every win_rate is 1: uniform
            return eligible[self.rng.gen_range(len(eligible))]
        sample = self.rng.gen_f64()
        cumsum = 0.0
        for i, w in enumerate(weights):
            cumsum += w / total
            if sample < cumsum:
                return eligible[i]
        return eligible[-1]

    def refresh_current_opponents(self):
        self.current_opponents = []
        if not self.available:
            return
        for _ in range(self.num_opponent_slots):
            idx = self.sample_opponent(list(self.current_opponents))
            if idx is not None:
                self.current_opponents.append(idx)

    def sample_all_slots(self):
        return list(self.current_opponents)

    # -- results (opponent_pool.rs:570-653) --------------------------------
    def queue_game_result(self, placements, learner_position, position_to_opponent):
        """placements[seat] (1 = first); position_to_opponent[seat] = pool index, None or a
        negative value on the learner's seat"""
        learner_placement = placements[learner_position]
        swiss = float(len(placements) - learner_placement)
        for pos, placement in enumerate(placements):
            if pos == learner_position:
                continue
            idx = position_to_opponent[pos]
            if idx is None or idx < 0:
                continue
            e = self.pending_rotation_stats.setdefault(int(idx), [0, 0, 0.0])
            e[1] += 1
            e[2] += swiss
            if learner_placement < placement:
                e[0] += 1

    def queue_results(self, wins, games, swiss, slot_to_pool):
        """the same, from the device's per-model-slot sums of a rollout
        (bppo_opponents_results); slot_to_pool[k] = pool index of device model slot k"""
        for k, idx in enumerate(slot_to_pool):
            if int(games[k]) == 0:
                continue
            e = self.pending_rotation_stats.setdefault(int(idx), [0, 0, 0.0])
            e[0] += int(wins[k])
            e[1] += int(games[k])
            e[2] += float(int(swiss[k]))

    def apply_pending_win_rate_updates(self):
        alpha = self.opponent_select_alpha
        pending, self.pending_rotation_stats = self.pending_rotation_stats, {}
        for idx, (wins, games, total_swiss) in pending.items():
            if games == 0 or not 0 <= idx < len(self.available):
                continue
            s = self.available[idx]
            s.win_rate = s.win_rate * (1.0 - alpha) + (wins / games) * alpha
            s.avg_swiss_points = s.avg_swiss_points * (1.0 - alpha) + (total_swiss / games) * alpha
            s.games_played += games

    # -- metrics (opponent_pool.rs:655-699, 890-947) -----------------------
    def compute_all_selection_probabilities(self):
        if not self.available:
            return []
        weights = [self._weight(s.win_rate) for s in self.available]
        total = 0.0
        for w in weights:
            total += w
        if total == 0.0:
            return [1.0 / len(self.available)] * len(self.available)
        return [w / total for w in weights]

    def get_best_checkpoint_index(self):
        """the checkpoint with the highest avg_swiss_points; Iterator::max_by returns the
        last of equal maxima"""
        if not self.available:
            return None
        best = 0
        for i, s in enumerate(self.available):
            if not s.avg_swiss_points < self.available[best].avg_swiss_points:
                best = i
        return best

    def get_pool_performance(self, num_players):
        """0.0 = the learner dominates the best checkpoint, 1.0 = it is dominated; None
        without games against it"""
        if not self.available or num_players < 2:
            return None
        best = self.available[self.get_best_checkpoint_index()]
        if best.games_played == 0:
            return None
        max_points = float(num_players - 1)
        score = (max_points - best.avg_swiss_points) / max_points
        return float(np.float32(min(max(score, 0.0), 1.0)))

    # -- persistence (opponent_pool.rs:167-183, 281-352) -------------------
    def save_opponent_stats(self, path):
        """OpponentStatsFile as serde_json::to_string_pretty writes it, temp file + rename"""
        doc = {"version": 1,
               "config": {"opponent_select_alpha": self.opponent_select_alpha,
                          "opponent_select_exponent": self.opponent_select_exponent},
               "opponents": [asdict(s) for s in self.available]}
        tmp = str(path) + ".tmp"
        with open(tmp, "w") as f:
            f.write(to_json_pretty(doc))
        os.replace(tmp, path)

    def load_opponent_stats(self, path):
        """the file's entries replace the statistics of the pool members they name; an entry
        the pool does not know yet is appended without a model (add_checkpoint supplies it).
        -> the file's config section"""
        with open(path) as f:
            doc = json.load(f)
        if "version" not in doc or "config" not in doc:
            raise ValueError(f"{path}: not an opponent_stats.json (version / config missing)")
        for o in doc["opponents"]:
            s = OpponentStats(o["checkpoint_name"], int(o["checkpoint_step"]), float(o["win_rate"]),
                              float(o.get("avg_swiss_points", 0.0)), int(o["games_played"]))
            for i, have in enumerate(self.available):
                if have.checkpoint_name == s.checkpoint_name:
                    self.available[i] = s
                    break
            else:
                self.available.append(s)
                self.models.append(None)
        return doc["config"]


class RatingHistory:
    """rating_history.rs:78-341 without the persistence and the graph: the games live in a
    rating table; player ids are the order of registration (ensure_checkpoint_registered)."""

    def __init__(self, device=0, backend=None):
        self.table = RatingTable(device=device)
        self.backend = backend or ("host" if device is None else "device")
        self.checkpoint_to_idx = {}
        self.idx_to_checkpoint = []
        self.idx_to_step = []
        self.first_checkpoint_idx = None
        self._current = None
        self.cached_ratings = None
        self.last_result = None

    def ensure_checkpoint_registered(self, name, step=0):
        idx = self.checkpoint_to_idx.get(name)
        if idx is not None:
            if step > 0 and self.idx_to_step[idx] == 0:
                self.idx_to_step[idx] = int(step)
            return idx
        idx = len(self.idx_to_checkpoint)
        self.checkpoint_to_idx[name] = idx
        self.idx_to_checkpoint.append(name)
        self.idx_to_step.append(int(step))
        return idx

    def on_checkpoint_saved(self, name, step):
        idx = self.ensure_checkpoint_registered(name, step)
        if self.first_checkpoint_idx is None:
            self.first_checkpoint_idx = idx
        self.idx_to_step[idx] = int(step)
        self._current = name
        self.cached_ratings = None

    @property
    def current_checkpoint(self):
        return self._current

    @property
    def total_games(self):
        return self.table.num_games

    def record_game(self, current, opponents, placements):
        """placements: [the learner's, then each opponent's] (rating_placements, ppo.rs:890-897)"""
        ids = [self.ensure_checkpoint_registered(current)] + [self.ensure_checkpoint_registered(o) for o in opponents]
        self.table.add_games([ids], [list(placements)])
        self.cached_ratings = None

    def record_rollout(self, ctx, slot_to_pool, pool):
        """main.rs:755-790 for every finished opponent game of ctx's last rollout, on the device:
        the learner plays under the current checkpoint's name ("step_00000000" before the first
        save), device model slot k under pool member slot_to_pool[k]'s; games against nothing but
        the current checkpoint are skipped.  The learner and every slot's checkpoint are
        registered, whether or not they finished a game.  -> games recorded"""
        learner = self.ensure_checkpoint_registered(self._current or "step_00000000")
        slots = [self.ensure_checkpoint_registered(pool.get_checkpoint_name(i)) for i in slot_to_pool]
        added = self.table.add_completions(ctx, learner, slots)
        if added:
            self.cached_ratings = None
        return added

    def compute_ratings(self):
        """rating_history.rs:270-341 -> {current_elo, best_elo, best_step, total_games}"""
        n = len(self.idx_to_checkpoint)
        total = self.total_games
        if n == 0 or total == 0:
            self.cached_ratings = []
            return dict(current_elo=1000.0, best_elo=1000.0, best_step=0, total_games=0)
        res = self.table.fit(n, 0, PlackettLuceConfig(), self.backend)
        self.last_result = res
        raw = [r.rating for r in res.ratings]
        first = self.first_checkpoint_idx if self.first_checkpoint_idx is not None else 0
        shift = 1000.0 - (raw[first] if first < n else 1000.0)
        adjusted = [r + shift for r in raw]
        best_idx, best = 0, -np.inf
        for i, r in enumerate(adjusted):
            if r > best:
                best, best_idx = r, i
        cur = max(n - 2, 0)
        self.cached_ratings = adjusted
        return dict(current_elo=adjusted[cur], best_elo=best, best_step=self.idx_to_step[best_idx], total_games=total)

    def close(self):
        self.table.close()


class PoolTrainer:
    """The opponent-pool branch of run_training's loop (main.rs:616-654, 729-803) on one
    context: envs [0, num_opponent_envs) play the pool's current opponents, the finished
    games' results feed the pool's win rates, and the opponents are re-drawn every update."""

    def __init__(self, cfg, pool, num_opponent_envs, device=0, params=None, init_seed=0, rating_history=None):
        if not pool.has_opponents():
            raise ValueError("PoolTrainer: the pool has no checkpoints")
        self.trainer = Trainer(cfg, device=device, params=params, init_seed=init_seed)
        self.ctx = self.trainer.ctx
        self.pool = pool
        self.rating_history = rating_history     # a RatingHistory fed by step() and add_checkpoint()
        self.n_opp = int(num_opponent_envs)
        P = self.ctx.seats
        if pool.num_opponent_slots != P - 1:
            raise ValueError(f"PoolTrainer: the pool draws {pool.num_opponent_slots} opponents per game, "
                             f"the env seats {P - 1}")
        if not pool.current_opponents:
            pool.refresh_current_opponents()
        # main.rs:640-651: EnvState::new per opponent env, seats drawn from the pool's RNG
        self.learner_pos = np.zeros(self.n_opp, np.int32)
        seat_pool = np.full((self.n_opp, P), -1, np.int64)      # pool index per seat
        for e in range(self.n_opp):
            assigned = pool.sample_all_slots()
            lp = pool.rng.gen_range(P)
            others = [p for p in range(P) if p != lp]
            pool.rng.shuffle(others)
            self.learner_pos[e] = lp
            for i, seat in enumerate(others):
                seat_pool[e, seat] = assigned[i]
        self.slot_to_pool = []
        self.pool_performance = None
        self.history = []                    # current_opponents of every update
        self._upload(seat_pool)

    # the device model slots = current_opponents and every opponent still seated in a
    # running game (unload_unused's in-use set, opponent_pool.rs:556-568), ascending
    def _upload(self, seat_pool):
        in_use = sorted(set(int(i) for i in self.pool.current_opponents) |
                        set(int(i) for i in seat_pool[seat_pool >= 0]))
        if len(in_use) > MAX_DEVICE_MODELS:
            raise RuntimeError(f"PoolTrainer: {len(in_use)} pool checkpoints are in use (current opponents and "
                               f"running games), the device holds {MAX_DEVICE_MODELS} models")
        missing = [self.pool.get_checkpoint_name(i) for i in in_use if self.pool.models[i] is None]
        if missing:
            raise RuntimeError(f"PoolTrainer: no model for {missing} (add_checkpoint supplies it)")
        slot_of = {idx: k for k, idx in enumerate(in_use)}
        p2o = np.full(seat_pool.shape, -1, np.int32)
        for idx, k in slot_of.items():
            p2o[seat_pool == idx] = k
        cur = np.array([slot_of[int(i)] for i in self.pool.current_opponents], np.int32)
        params = np.stack([self.pool.models[i][0] for i in in_use])
        self.ctx.set_opponents(params, [self.pool.models[i][1] for i in in_use], self.n_opp, self.learner_pos,
                               p2o, cur)
        self.slot_to_pool = in_use

    def device_slots(self):
        return list(self.slot_to_pool)

    def add_checkpoint(self, name, step, normalizer=None):
        """the learner's current parameters join the pool (main.rs: after a checkpoint save)"""
        self.pool.add_checkpoint(name, step, self.trainer.model.get_params(), normalizer)
        if self.rating_history is not None:
            self.rating_history.on_checkpoint_saved(name, step)

    def step(self):
        """one update: rollout against the current opponents, GAE, PPO update, then
        queue_game_result over the finished games, apply_pending_win_rate_updates,
        eval/pool_performance and refresh_current_opponents.  -> the update's metrics"""
        tr = self.trainer
        lr = schedule_get(tr.cfg["learning_rate"], tr.global_step)
        ent = schedule_get(tr.cfg["entropy_coef"], tr.global_step)
        tr.vec_env.set_step(tr.global_step)
        info, metrics = train_step(self.ctx, lr, ent)
        tr.global_step += tr.steps_per_update
        wins, games, swiss = self.ctx.opponent_results()
        self.pool.queue_results(wins, games, swiss, self.slot_to_pool)
        self.pool.apply_pending_win_rate_updates()
        self.pool_performance = self.pool.get_pool_performance(self.ctx.num_players)
        self.pool.refresh_current_opponents()
        self.history.append(list(self.pool.current_opponents))
        if self.rating_history is not None:      # before the re-upload empties the records
            metrics["rated_games"] = self.rating_history.record_rollout(self.ctx, self.slot_to_pool, self.pool)
        # the seats stay as the rollout left them; only the slot numbering may change
        lp, p2o = self.ctx.opponent_envs()
        self.learner_pos = lp.copy()
        old = np.array(self.slot_to_pool, np.int64)
        seat_pool = np.where(p2o >= 0, old[np.maximum(p2o, 0)], -1)
        self._upload(seat_pool)
        metrics["episodes"] = info.episodes
        metrics["mean_return"] = info.mean_return
        metrics["opponent_games"] = int(np.sum(games))
        metrics["pool_performance"] = self.pool_performance
        return metrics

    def close(self):
        self.trainer.close()
