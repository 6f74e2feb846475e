"""Tournaments on the device (tournament.rs), host side only.

    round_robin_pods        tournament.rs:918-920
    swiss_points            tournament.rs:715-750 calculate_swiss_points
    run_round               the pods of a round through bppo.eval.evaluate_pods; per pod the
                            MatchupGames content of run_pod (tournament.rs:1788-1870)

    find_anchor_index       tournament.rs:1017-1033
    rate_round              compute_ratings(contestants, all_games), tournament.rs:1035-1049, on a
                            device rating table (bppo.ratings)

    Contestant              tournament.rs:121-155
    pod_avg_points, pod_full_draws, pod_summary
                            MatchupGames::avg_points / full_draws / summary, tournament.rs:54-106
    has_repeat_opponents    tournament.rs:753-762
    swiss_pods              tournament.rs:771-834
    form_dutch_pods, form_dutch_pods_with_floaters
                            tournament.rs:838-911
    update_stats_from_games tournament.rs:929-1013
    assign_byes             the bye block of the round loop, tournament.rs:2089-2120
    tournament_format       tournament.rs:2025-2035
    run_tournament          run_tournament_env's round loop, tournament.rs:2062-2296
    TournamentResult.results
                            build_results, tournament.rs:184-236, 1695-1776

Every pod has its own RNG (evaluate_pods), where the reference hands one StdRng from pod to
pod: run_tournament draws one u64 per pod from StdRng(seed) in play order and seeds the pod
with it.  Checkpoint discovery on disk, display names, the graphs and
the progress bars are not part of this module."""
import itertools
import math
import sys
import time
from dataclasses import dataclass, field

from .eval import TempSchedule, evaluate_pods, evaluate_pods_ctx
from .ratings import RatingTable
from .rng import StdRng


def round_robin_pods(n, pod_size):
    """every combination of pod_size contestants out of n, in lexicographic order"""
    return [list(p) for p in itertools.combinations(range(n), pod_size)]


def swiss_points(placements):
    """points of one game by fractional ranking: N - the average of the positions a tie group
    occupies.  [1, 1, 3, 4] -> [2.5, 2.5, 1.0, 0.0]"""
    n = len(placements)
    counts = {}
    for p in placements:
        counts[p] = counts.get(p, 0) + 1
    avg, pos = {}, 1
    for p in sorted(counts):
        avg[p] = (pos + (pos + counts[p] - 1)) / 2.0
        pos += counts[p]
    return [float(n) - avg[p] for p in placements]


def run_round(config, models, normalizers, pods, num_games, envs_per_pod, temp_schedule=None, seeds=None, seed=0,
              device=0, max_steps=None):
    """pods[k]: the contestants of pod k, indices into models (None = the random player).
    -> per pod {"contestants": pods[k], "games": [placements of each game, per contestant],
    "stats": its EvalStats}"""
    stats = evaluate_pods(config, models, normalizers, pods, num_games, envs_per_pod, temp_schedule, seeds, seed,
                          device, max_steps)
    return [{"contestants": list(pod), "games": [list(o) for o in st.game_outcomes], "stats": st}
            for pod, st in zip(pods, stats)]


def find_anchor_index(names):
    """the anchor of a tournament's ratings: the contestant called "Random" if there is one, else
    the "step_*" contestant with the smallest name (the first of equal ones), else None"""
    for i, n in enumerate(names):
        if n == "Random":
            return i
    best = None
    for i, n in enumerate(names):
        if n.startswith("step_") and (best is None or n < names[best]):
            best = i
    return best


def rate_round(results, n_contestants, anchor, table=None, random_index=None, config=None, device=0,
               backend="device"):
    """Append the games of run_round's output to a rating table and fit it over n_contestants
    players: a pod's contestant indices are the player ids as they are; a None contestant (the
    random player) is player random_index, as the caller numbers it.  table: a RatingTable that
    already holds the earlier rounds' games (the reference refits over all games after every
    round, tournament.rs:2250); None = a table of this call's own.  -> RatingResult"""
    own = table is None
    if own:
        table = RatingTable(device=device)
    try:
        players, placements = [], []
        for pod in results:
            ids = []
            for c in pod["contestants"]:
                if c is None:
                    if random_index is None:
                        raise ValueError("rate_round: a pod seats the random player (None); give random_index")
                    c = random_index
                ids.append(int(c))
            for game in pod["games"]:
                players.append(ids)
                placements.append([int(p) for p in game])
        table.add_games(players, placements)
        return table.fit(n_contestants, anchor, config, backend)
    finally:
        if own:
            table.close()


# ------------------------------------------------------------- contestants ---
@dataclass
class Contestant:
    """tournament.rs:121-155.  model: index into run_tournament's models, None = the random
    player; source: the checkpoint's path as text (PlayerSource::Checkpoint), None otherwise"""
    name: str
    model: object = None
    initial_seed: float = 0.0
    opponents_faced: list = field(default_factory=list)
    placement_counts: list = field(default_factory=list)
    games_played: int = 0
    draw_count: int = 0
    swiss_points: float = 0.0
    has_bye: bool = False
    source: object = None

    def wins(self):
        """1st places without the draws (tournament.rs:158-165)"""
        return max((self.placement_counts[0] if self.placement_counts else 0) - self.draw_count, 0)

    def losses(self):
        """last places (tournament.rs:168-175)"""
        return self.placement_counts[-1] if len(self.placement_counts) >= 2 else 0

    def draws(self):
        return self.draw_count


# -------------------------------------------------------------- pod results ---
def pod_avg_points(games, idx):
    """MatchupGames::avg_points (tournament.rs:54-70): the mean over the pod's games of seat
    idx's Swiss points; 0 without games"""
    if not games:
        return 0.0
    total = 0.0
    for g in games:
        pts = swiss_points(g)
        total += pts[idx] if idx < len(pts) else 0.0
    return total / float(len(games))


def pod_full_draws(games):
    """MatchupGames::full_draws (tournament.rs:73-78): games in which everybody placed 1st"""
    return sum(1 for g in games if len(g) and all(p == 1 for p in g))


def pod_summary(games, names):
    """MatchupGames::summary (tournament.rs:81-106): "A vs B: 0.67-0.33 (A)" """
    points = [pod_avg_points(games, i) for i in range(len(names))]
    best = 0
    for i, p in enumerate(points):          # max_by: the last of equal maxima
        if p >= points[best]:
            best = i
    if not points or all(abs(p - points[0]) < 0.001 for p in points):
        winner = "draw"
    else:
        winner = names[best]
    return f"{' vs '.join(names)}: {'-'.join(f'{p:.2f}' for p in points)} ({winner})"


# ------------------------------------------------------------------ pairing ---
def has_repeat_opponents(pod, contestants):
    """tournament.rs:753-762: whether a pair of the pod has met (the earlier one's list is read)"""
    for i in range(len(pod)):
        for j in range(i + 1, len(pod)):
            if pod[j] in contestants[pod[i]].opponents_faced:
                return True
    return False


def form_dutch_pods_with_floaters(ranked_indices, pod_size, contestants):
    """tournament.rs:849-911: the ranked list cut into pod_size groups of num_pods, pod i takes
    the i-th of every group; a pod with a repeat pairing tries the later players of the last
    group in turn and swaps with the first that leaves no repeat.  -> (pods, floaters: the
    players past num_pods * pod_size)"""
    ranked_indices = list(ranked_indices)
    if len(ranked_indices) < pod_size:
        return [], ranked_indices
    num_pods = len(ranked_indices) // pod_size
    if num_pods == 0:
        return [], ranked_indices
    indices = list(ranked_indices)
    pods = []
    for pod_idx in range(num_pods):
        pod = [indices[pod_idx + group * num_pods] for group in range(pod_size)
               if pod_idx + group * num_pods < len(indices)]
        if len(pod) == pod_size and has_repeat_opponents(pod, contestants):
            current_last_pos = pod_idx + (pod_size - 1) * num_pods
            for swap_offset in range(1, num_pods - pod_idx):
                swap_pos = current_last_pos + swap_offset
                if swap_pos < len(indices):
                    test_pod = pod[:pod_size - 1] + [indices[swap_pos]]
                    if not has_repeat_opponents(test_pod, contestants):
                        indices[current_last_pos], indices[swap_pos] = indices[swap_pos], indices[current_last_pos]
                        pod = test_pod
                        break
        if len(pod) == pod_size:
            pods.append(pod)
    return pods, indices[num_pods * pod_size:]


def form_dutch_pods(ranked_indices, pod_size, contestants):
    """tournament.rs:838-845"""
    return form_dutch_pods_with_floaters(ranked_indices, pod_size, contestants)[0]


def swiss_pods(contestants, pod_size):
    """tournament.rs:771-834.  Round 1 (every swiss_points == 0): ranked by initial_seed,
    descending.  Later rounds: ranked by (swiss_points, initial_seed) descending, cut into score
    brackets where the points step by more than 0.001; a bracket's floaters join the next
    bracket at its top; the last bracket's floaters do not play.  (The sorts are stable, as
    Rust's sort_by.)"""
    n = len(contestants)
    if n < pod_size:
        return []
    if all(c.swiss_points == 0.0 for c in contestants):
        ranked = sorted(range(n), key=lambda i: -contestants[i].initial_seed)
        return form_dutch_pods(ranked, pod_size, contestants)
    ranked = sorted(range(n), key=lambda i: (-contestants[i].swiss_points, -contestants[i].initial_seed))
    brackets, current_score = [], sys.float_info.max
    for i in ranked:
        points = contestants[i].swiss_points
        if abs(points - current_score) > 0.001:
            brackets.append([])
            current_score = points
        brackets[-1].append(i)
    all_pods, floaters = [], []
    for bracket in brackets:
        pods, floaters = form_dutch_pods_with_floaters(floaters + bracket, pod_size, contestants)
        all_pods.extend(pods)
    return all_pods


def assign_byes(contestants, pod_size):
    """tournament.rs:2089-2120: len % pod_size byes, to the lowest by (swiss_points,
    initial_seed) among those without a bye yet; each is worth pod_size - 1 points and sets
    has_bye.  -> the recipients' indices in that order"""
    num_byes = len(contestants) % pod_size
    recipients = []
    if num_byes > 0:
        cand = sorted((i for i, c in enumerate(contestants) if not c.has_bye),
                      key=lambda i: (contestants[i].swiss_points, contestants[i].initial_seed))
        for i in cand[:num_byes]:
            contestants[i].swiss_points += float(pod_size - 1)
            contestants[i].has_bye = True
            recipients.append(i)
    return recipients


def round_pods(contestants, pod_size):
    """One Swiss round's byes and pods (tournament.rs:2089-2136): the byes are awarded, the
    rest paired by swiss_pods among themselves, indices mapped back.  -> (byes, pods)"""
    byes = assign_byes(contestants, pod_size)
    active = [i for i in range(len(contestants)) if i not in byes]
    pods = swiss_pods([contestants[i] for i in active], pod_size)
    # as the reference: it pairs clones of the active contestants by their position among the
    # active ones, while their opponents_faced still list indices of the full table, so after
    # a bye the repeat check compares the two numberings (tournament.rs:2127-2136, 753-762)
    return byes, [[active[i] for i in pod] for pod in pods]


def update_stats_from_games(contestants, pod, games):
    """tournament.rs:929-1013: per game the placement counts, draws (all placements equal) and
    games played; the games' Swiss points summed per seat; the match placements by those sums
    (ties within f64::EPSILON share a place); the Swiss points of the match placements added
    to swiss_points; opponents_faced in first-met order"""
    if not games:
        return
    n = len(pod)
    raw = [0.0] * n
    for g in games:
        is_draw = all(g[k] == g[k + 1] for k in range(len(g) - 1))
        for i, ci in enumerate(pod):
            c = contestants[ci]
            if len(c.placement_counts) < n:
                c.placement_counts.extend([0] * (n - len(c.placement_counts)))
            if 0 < g[i] <= n:
                c.placement_counts[g[i] - 1] += 1
            if is_draw:
                c.draw_count += 1
            c.games_played += 1
        for i, pts in enumerate(swiss_points(g)):
            raw[i] += pts
    order = sorted(range(n), key=lambda i: -raw[i])
    match_placements = [0] * n
    place, i = 1, 0
    while i < n:
        j = i
        while j < n and abs(raw[order[j]] - raw[order[i]]) < sys.float_info.epsilon:
            j += 1
        for k in range(i, j):
            match_placements[order[k]] = place
        place = j + 1
        i = j
    for i, pts in enumerate(swiss_points(match_placements)):
        contestants[pod[i]].swiss_points += pts
    for ci in pod:
        for oi in pod:
            if ci != oi and oi not in contestants[ci].opponents_faced:
                contestants[ci].opponents_faced.append(oi)


def tournament_format(n, pod_size, format="auto", rounds=None):
    """tournament.rs:2025-2035: Swiss iff there are more than 50 matchups C(n, pod_size) and
    round-robin was not asked for, with ceil(log2 n) + 1 rounds unless given; round-robin is
    one round.  format "swiss" forces Swiss pairing (small tournaments).  -> (use_swiss, rounds)"""
    if format not in ("auto", "swiss", "round-robin"):
        raise ValueError('format: "auto", "swiss" or "round-robin"')
    use_swiss = format == "swiss" or (format == "auto" and math.comb(n, pod_size) > 50)
    if not use_swiss:
        return False, 1
    return True, int(rounds) if rounds is not None else int(math.ceil(math.log2(float(n)))) + 1


def standings_order(contestants):
    """print_standings' and build_results' order (tournament.rs:1062-1073, 1705-1715): by
    (swiss_points, initial_seed) descending, stable"""
    return sorted(range(len(contestants)), key=lambda i: (-contestants[i].swiss_points, -contestants[i].initial_seed))


# ------------------------------------------------------------------- engine ---
MAX_MODELS_PER_CALL = 64      # bppo_evaluate_pods' limits
MAX_PODS_PER_CALL = 1024


def split_round(pod_models, max_models=MAX_MODELS_PER_CALL, max_pods=MAX_PODS_PER_CALL):
    """A round cut into device calls, greedily in pod order: a call takes pods while it has at
    most max_pods of them and max_models distinct models, the random player counted as one.
    pod_models[k]: the models of pod k.  -> [(first pod, end pod)]"""
    calls, start, seen = [], 0, set()
    for k, ms in enumerate(pod_models):
        new = set(ms)
        if len(new) > max_models:
            raise ValueError(f"pod {k} alone seats more than {max_models} distinct models")
        if k > start and (len(seen | new) > max_models or k - start >= max_pods):
            calls.append((start, k))
            start, seen = k, set()
        seen |= new
    if len(pod_models) > start:
        calls.append((start, len(pod_models)))
    return calls


class DeviceEngine:
    """The default engine of run_tournament: engine(pods, pod_seeds) plays the pods (contestant
    indices) through bppo_evaluate_pods, one call per split_round piece; a context is kept per
    call size and reused by later calls and rounds.  close() frees them."""

    def __init__(self, config, contestant_model, models, normalizers, num_games, envs_per_pod, temp_schedule,
                 device=0, max_steps=None, max_models_per_call=MAX_MODELS_PER_CALL):
        self.config, self.contestant_model = dict(config), list(contestant_model)
        self.models, self.normalizers = models, normalizers
        self.num_games, self.envs_per_pod, self.temp_schedule = int(num_games), int(envs_per_pod), temp_schedule
        self.device, self.max_steps = device, max_steps
        self.max_models = min(int(max_models_per_call), MAX_MODELS_PER_CALL)
        self.calls = []               # (pods, distinct models) of every device call so far
        self._ctx = {}

    def _context(self, n_pods):
        from .ppo import Context
        if n_pods not in self._ctx:
            cfg = dict(self.config)
            cfg["num_envs"] = n_pods * self.envs_per_pod
            self._ctx[n_pods] = Context(cfg, device=self.device)
        return self._ctx[n_pods]

    def close(self):
        for ctx in self._ctx.values():
            ctx.close()
        self._ctx = {}

    def __call__(self, pods, pod_seeds):
        pod_models = [[self.contestant_model[c] for c in pod] for pod in pods]
        out = []
        for a, b in split_round(pod_models, self.max_models):
            local = []                # the call's distinct models, first-met order
            for ms in pod_models[a:b]:
                for m in ms:
                    if m not in local:
                        local.append(m)
            params = [None if m is None else self.models[m] for m in local]
            norms = [None if m is None or not self.normalizers else self.normalizers[m] for m in local]
            seats = [[local.index(m) for m in ms] for ms in pod_models[a:b]]
            res = evaluate_pods_ctx(self._context(b - a), params, norms, seats, self.num_games, self.envs_per_pod,
                                    self.temp_schedule, pod_seeds[a:b], self.max_steps)
            self.calls.append((b - a, len(local)))
            P = len(pods[a])
            out.extend([[int(x) for x in g["placement"][:P]] for g in rec] for rec, _ in res)
        return out


# --------------------------------------------------------------- tournament ---
@dataclass
class TournamentResult:
    contestants: list
    pods: list                   # (round, contestant indices, games: the placements of each game)
    byes: list                   # per round the bye recipients
    ratings: object              # bppo.ratings.RatingResult
    num_rounds: int = 1
    use_swiss: bool = False
    num_games: int = 0
    temp: object = None          # the schedule's initial temperature when one was given
    seed: object = None
    environment: str = ""
    pod_seeds: list = field(default_factory=list)

    def standings(self):
        """contestant indices in print_standings' order"""
        return standings_order(self.contestants)

    def results(self, timestamp=None):
        """build_results (tournament.rs:1695-1776) as a dict in TournamentResults' field order
        (tournament.rs:184-236); source, temp and seed are left out when None"""
        from .checkpoint import F32
        rankings = []
        for rank, i in enumerate(self.standings()):
            c, r = self.contestants[i], self.ratings.ratings[i]
            e = {"rank": rank + 1, "name": c.name}
            if c.source is not None:
                e["source"] = str(c.source)
            e.update(swiss_points=float(c.swiss_points), rating=float(r.rating), uncertainty=float(r.uncertainty),
                     rating_low=r.rating - 2.0 * r.uncertainty, rating_high=r.rating + 2.0 * r.uncertainty,
                     placement_counts=[int(x) for x in c.placement_counts], draw_count=int(c.draw_count),
                     games_played=int(c.games_played))
            rankings.append(e)
        pods = [{"round": int(rnd), "contestants": [self.contestants[i].name for i in pod],
                 "avg_points": [pod_avg_points(games, k) for k in range(len(pod))], "games": len(games),
                 "draws": pod_full_draws(games)} for rnd, pod, games in self.pods]
        config = {"num_games_per_matchup": int(self.num_games), "num_rounds": int(self.num_rounds),
                  "format": "swiss" if self.use_swiss else "round-robin"}
        if self.temp is not None:
            config["temp"] = F32(self.temp)
        if self.seed is not None:
            config["seed"] = int(self.seed)
        if timestamp is None:
            timestamp = f"unix:{int(time.time())}"      # chrono_lite_now, tournament.rs:1779-1785
        return {"rankings": rankings, "pods": pods, "config": config, "environment": self.environment,
                "timestamp": timestamp}

    def results_json(self, timestamp=None):
        """serde_json::to_string_pretty of results()"""
        from .checkpoint import to_json_pretty
        return to_json_pretty(self.results(timestamp))


def compute_tournament_ratings(contestants, all_games, device=0, backend="device"):
    """compute_ratings (tournament.rs:1035-1049) over [(contestant indices, placements)]: the
    anchor is find_anchor_index, else the last contestant"""
    anchor = find_anchor_index([c.name for c in contestants])
    if anchor is None:
        anchor = max(len(contestants) - 1, 0)
    table = RatingTable(device=None if backend == "host" else device)
    try:
        table.add_games([g[0] for g in all_games], [g[1] for g in all_games])
        return table.fit(len(contestants), anchor, None, backend)
    finally:
        table.close()


def run_tournament(config, contestants, models, normalizers, num_games, envs_per_pod, temp_schedule=None, seed=0,
                   rounds=None, format="auto", device=0, max_steps=None, engine=None, rating_backend="device",
                   max_models_per_call=MAX_MODELS_PER_CALL):
    """run_tournament_env's round loop (tournament.rs:2062-2296) over contestants (their
    statistics are updated in place; contestant.model indexes models / normalizers, None = the
    random player).  Swiss: per round assign_byes, swiss_pods over the others, the pods played,
    update_stats_from_games pod by pod in pod order; round-robin: one round of
    round_robin_pods.  At the end the Plackett-Luce ratings over all games.

    Seeds: StdRng(seed) gives one next_u64() per pod in play order, round by round, as that
    pod's seed.  The reference instead hands the one StdRng(seed) itself from pod to pod, so
    a pod's draws depend on how many words the pods before it consumed; pods that run side by
    side cannot keep that order (DESIGN.md sections 7e, 7h).

    engine(pods, pod_seeds) -> per pod the list of each game's placements; None = a
    DeviceEngine (bppo_evaluate_pods), which cuts a round into several calls when it seats more
    than max_models_per_call (at most 64) distinct models, the random player counted, or more
    than 1,024 pods.  models, normalizers, envs_per_pod, max_steps and max_models_per_call
    configure that default engine only: an engine that is passed in brings its own, and they
    are ignored (device still places the rating table).  rating_backend: "device" or "host"
    (bppo.ratings).  -> TournamentResult"""
    from .host import num_players
    n = len(contestants)
    pod_size = int(config.get("player_count", 4)) if config["env"] == "skull" else num_players(config["env"])
    use_swiss, num_rounds = tournament_format(n, pod_size, format, rounds)
    given_temp = temp_schedule is not None
    if temp_schedule is None:
        temp_schedule = TempSchedule.env_default(config["env"])
    own = engine is None
    if own:
        engine = DeviceEngine(config, [c.model for c in contestants], models, normalizers, num_games, envs_per_pod,
                              temp_schedule, device, max_steps, max_models_per_call)
    rng = StdRng.seed_from_u64(seed)
    all_pods, all_byes, all_games, all_seeds = [], [], [], []
    try:
        for rnd in range(1, num_rounds + 1):
            if use_swiss:
                byes, pods = round_pods(contestants, pod_size)
                if not pods and not byes:
                    break                                   # "No pods possible", tournament.rs:2138-2141
            else:
                byes, pods = [], round_robin_pods(n, pod_size)
            all_byes.append(byes)
            pod_seeds = [rng.next_u64() for _ in pods]
            played = engine(pods, pod_seeds) if pods else []
            if len(played) != len(pods):
                raise ValueError("engine: one result per pod")
            for pod, games, ps in zip(pods, played, pod_seeds):
                games = [[int(p) for p in g] for g in games]
                all_games.extend((list(pod), g) for g in games)
                update_stats_from_games(contestants, pod, games)
                all_pods.append((rnd, list(pod), games))
                all_seeds.append(ps)
    finally:
        if own:
            engine.close()
    ratings = compute_tournament_ratings(contestants, all_games, device, rating_backend)
    return TournamentResult(contestants=contestants, pods=all_pods, byes=all_byes, ratings=ratings,
                            num_rounds=num_rounds, use_swiss=use_swiss, num_games=int(num_games),
                            temp=float(temp_schedule.initial) if given_temp else None, seed=seed,
                            environment=config["env"], pod_seeds=all_seeds)
