"""Python restatement of the reference's stats-mode evaluation (eval.rs) on the CPU
oracle's primitives.  TEST INFRASTRUCTURE ONLY: the parity checker of bppo_evaluate.

    TempSchedule.get_temp        eval.rs:200-216
    sample_with_temperature      eval.rs:223-272
    rewards_to_placements        eval.rs:276-306
    generate_permutations        eval.rs:1591-1612
    run_stats_mode_env           eval.rs:1621-1877 over VecEnv (env.rs:281-487)

Envs are the oracle's per-env structs (E::new + reset + reset, the outcome read before the
auto-reset), logits come from or_net_forward / or_obs_norm_normalize_batch, RNG words from
or_rng_next_u32, expf and fmaf from the platform libm."""
import ctypes as C
import math

import numpy as np

import oracle_ffi as O

f32 = np.float32
_libm = C.CDLL("libm.so.6")
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
NEG_INF = f32(-np.inf)


# ------------------------------------------------------------ TempSchedule ---
class TempSchedule:
    def __init__(self, initial, final_temp=0.0, cutoff=None, decay=False):
        self.initial, self.final_temp = f32(initial), f32(final_temp)
        self.cutoff, self.decay = cutoff, bool(decay)

    def get_temp(self, move_num):
        if self.cutoff is None:
            return self.initial
        if move_num >= self.cutoff:
            return self.final_temp
        if not self.decay:
            return self.initial
        t = f32(move_num) / f32(self.cutoff)
        return f32(_libm.fmaf(float(t), float(self.final_temp - self.initial), float(self.initial)))   # mul_add


# ------------------------------------------------- sample_with_temperature ---
def word_to_f32(w):
    """rand 0.8.5 Standard f32 (restated, verify): 24 high bits of one word times 2^-24"""
    return f32(int(w) >> 8) * f32(2.0 ** -24)


def sample_with_temperature(logits, mask, temperature, next_u32):
    """-> (action, draws used).  mask: None or a bool/0-1 sequence; next_u32(): the RNG."""
    A = len(logits)
    if mask is not None:
        x = [f32(l) if m else NEG_INF for l, m in zip(logits, mask)]
    else:
        x = [f32(l) for l in logits]
    temperature = f32(temperature)
    if temperature == 0.0:
        best, bv = 0, x[0]           # max_by(partial_cmp.unwrap_or(Equal)): the last of equal maxima
        for a in range(1, A):
            if not (bv > x[a]):
                best, bv = a, x[a]
        return best, 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        scaled = [v / temperature for v in x]
        mx = NEG_INF                 # fold(NEG_INFINITY, f32::max): a NaN side is ignored
        for v in scaled:
            if math.isnan(mx) or v > mx:
                mx = v
        ex = [f32(_libm.expf(float(v - mx))) for v in scaled]
        s = f32(0.0)
        for v in ex:
            s = f32(s + v)
        if s == 0.0:
            if mask is not None:
                for a in range(A):
                    if mask[a]:
                        return a, 0
            return 0, 0
        probs = [v / s for v in ex]
        r = word_to_f32(next_u32())
        cum = f32(0.0)
        for a in range(A):
            cum = f32(cum + probs[a])
            if r < cum:
                return a, 1
        return A - 1, 1


def rewards_to_placements(rewards):
    r = [f32(v) for v in rewards]
    idx = sorted(range(len(r)), key=lambda i: -r[i])        # stable sort, descending
    pl = [0] * len(r)
    cur, i = 1, 0
    while i < len(idx):
        first, tied = r[idx[i]], 0
        while i + tied < len(idx) and abs(f32(r[idx[i + tied]] - first)) < f32(1e-6):
            tied += 1
        for j in range(tied):
            pl[idx[i + j]] = cur
        cur += tied
        i += tied
    return pl


def generate_permutations(n):
    result, arr = [], list(range(n))

    def heap_permute(k):
        if k == 1:
            result.append(list(arr))
            return
        heap_permute(k - 1)
        for i in range(k - 1):
            if k % 2 == 0:
                arr[i], arr[k - 1] = arr[k - 1], arr[i]
            else:
                arr[0], arr[k - 1] = arr[k - 1], arr[0]
            heap_permute(k - 1)

    heap_permute(n)
    return result


# -------------------------------------------------------------------- envs ---
class _C4:
    D, A, P = 86, 7, 2

    def __init__(self, seed, players):
        self.L = O.lib()
        self.e = O.ConnectFour()
        self.L.or_c4_new(C.byref(self.e))              # E::new ignores the seed
        self._obs = np.zeros(self.D, f32)
        self._r = np.zeros(2, f32)

    def set_num_players(self, n):
        pass

    def reset(self):
        self.L.or_c4_reset(C.byref(self.e), self._obs)

    def obs(self):
        self.L.or_c4_get_obs(C.byref(self.e), self._obs)
        return self._obs

    def mask(self):
        m = np.zeros(self.A, np.uint8)
        self.L.or_c4_mask(C.byref(self.e), m)
        return m

    def player(self):
        return self.e.current - 1

    def step(self, a):
        d = C.c_int()
        self.L.or_c4_step(C.byref(self.e), int(a), self._obs, self._r, C.byref(d))
        return self._r.copy(), bool(d.value)

    def outcome(self):                                  # connect_four.rs:301-310
        if not self.e.game_over:
            return None
        return {1: [1, 2], 2: [2, 1]}.get(self.e.winner, [1, 1])


class _LD:
    D, A, P = 270, 49, 4

    def __init__(self, seed, players):
        self.L = O.lib()
        self.e = O.LiarsDice()
        self.L.or_ld_new(C.byref(self.e), seed)         # new_with_config rolls once
        self._obs = np.zeros(self.D, f32)
        self._r = np.zeros(4, f32)

    def set_num_players(self, n):
        pass

    def reset(self):
        self.L.or_ld_reset(C.byref(self.e), self._obs)

    def obs(self):
        self.L.or_ld_get_obs(C.byref(self.e), self._obs)
        return self._obs

    def mask(self):
        m = np.zeros(self.A, np.uint8)
        self.L.or_ld_mask(C.byref(self.e), m)
        return m

    def player(self):
        return self.e.current

    def step(self, a):
        d = C.c_int()
        self.L.or_ld_step(C.byref(self.e), int(a), 0.0, self._obs, self._r, C.byref(d))   # E::new: no shaping
        return self._r.copy(), bool(d.value)

    def outcome(self):                                  # liars_dice.rs:586-601
        if not self.e.game_over:
            return None
        pl = [0] * 4
        for order in range(self.e.num_elim):
            pl[self.e.elim_order[order]] = 4 - order
        return pl


class _SK:
    D, A, P = 135, 33, 6

    def __init__(self, seed, players):
        self.L = O.lib()
        self.e = O.Skull()
        self.L.or_skull_new(C.byref(self.e), 4, seed)   # E::new: 4 players (skull.rs:1062-1065)
        self._obs = np.zeros(self.D, f32)
        self._r = np.zeros(6, f32)

    def set_num_players(self, n):                       # skull.rs:1464-1470
        self.e.n = n

    def reset(self):
        self.L.or_skull_reset(C.byref(self.e), None)

    def obs(self):
        self.L.or_skull_get_obs(C.byref(self.e), self._obs)
        return self._obs

    def mask(self):
        m = np.zeros(self.A, np.uint8)
        self.L.or_skull_mask(C.byref(self.e), m)
        return m

    def player(self):
        return self.e.current

    def step(self, a):
        d, inv = C.c_int(), C.c_int()
        self.L.or_skull_step(C.byref(self.e), int(a), 0.0, None, self._r, C.byref(d), C.byref(inv))
        assert not inv.value, "action outside the mask"
        return self._r.copy(), bool(d.value)

    def outcome(self):                                  # skull.rs:1338-1343
        if not self.e.game_over:
            return None
        out = np.zeros(6, np.int32)
        self.L.or_skull_outcome(C.byref(self.e), out)
        return [int(v) for v in out]


ENVS = {"connect_four": _C4, "liars_dice": _LD, "skull": _SK}


class Model:
    """one evaluated model: an oracle net description + flat parameters + optional
    ObsNormalizer state (mean, m2, count); Model.random() is the reference's None"""

    def __init__(self, desc, params, norm=None):
        self.desc, self.params, self.norm = desc, None if params is None else np.ascontiguousarray(params, f32), norm
        self._on = None
        if norm is not None and norm[2] >= 2.0:
            mean, m2, count = norm
            self._on = O.ObsNorm()
            O.lib().or_obs_norm_init(C.byref(self._on), len(mean), 10.0)
            for i in range(len(mean)):
                self._on.mean[i] = float(mean[i])
                self._on.var[i] = float(m2[i])
            self._on.count = float(count)

    @classmethod
    def random(cls):
        return cls(None, None)

    def logits(self, obs):
        B = obs.shape[0]
        if self.params is None:
            return np.zeros((B, 0), f32)
        x = np.ascontiguousarray(obs, f32).copy()
        if self._on is not None:
            O.lib().or_obs_norm_normalize_batch(C.byref(self._on), x.reshape(-1), B)
        priv = np.zeros((B, self.desc.priv_dim), f32) if self.desc.priv_dim else None
        return O.net_forward(self.desc, self.params, x, priv)[0]


def run_stats_mode(env, num_envs, num_players, models, seat_model, num_games, sched, seed, max_steps=100000):
    """run_stats_mode_env.  -> dict: games [(total_reward[6] f32, placement[6], length, env_index,
    perm_index, step)], rng_pos, placements [checkpoint][place - 1], steps, ended_by"""
    L = O.lib()
    E = ENVS[env]
    rng = O.new_rng(seed)
    base_seed = L.or_rng_next_u64(C.byref(rng))
    envs = [E((base_seed + i) & 0xFFFFFFFFFFFFFFFF, num_players) for i in range(num_envs)]
    for e in envs:                       # VecEnv::new
        e.reset()
    for e in envs:                       # set_all_num_players
        e.set_num_players(num_players)
        e.reset()
    ep_rewards = [[f32(0.0)] * E.P for _ in range(num_envs)]
    ep_len = [0] * num_envs
    terminal = [False] * num_envs
    move_counts = [0] * num_envs
    perms = generate_permutations(num_players)
    perm_idx = [i % len(perms) for i in range(num_envs)]
    ncp = len(seat_model)
    assert ncp == num_players
    games, placements = [], np.zeros((ncp, ncp), np.int64)
    completed, step, ended_by = 0, 0, "num_games"

    def next_u32():
        return L.or_rng_next_u32(C.byref(rng))

    while completed < num_games:
        if all(terminal):
            ended_by = "no active env"
            break
        assert step < max_steps, "max_steps"
        players = [e.player() for e in envs]
        actions = [0] * num_envs
        for mi, model in enumerate(models):
            idx = [i for i in range(num_envs) if not terminal[i]
                   and seat_model[perms[perm_idx[i]][players[i]]] == mi]
            if not idx:
                continue
            masks = [envs[i].mask() for i in idx]
            if model.params is None:
                logits = np.zeros((len(idx), E.A), f32)
            else:
                logits = model.logits(np.stack([envs[i].obs().copy() for i in idx]))
            for k, i in enumerate(idx):
                temp = sched.get_temp(move_counts[i])
                actions[i], _ = sample_with_temperature(logits[k], masks[k], temp, next_u32)
        done_envs = []
        for i, e in enumerate(envs):     # VecEnv::step
            if terminal[i]:
                continue
            r, done = e.step(actions[i])
            for p in range(E.P):
                ep_rewards[i][p] = f32(ep_rewards[i][p] + r[p])
            ep_len[i] += 1
            if done:
                done_envs.append((i, list(ep_rewards[i]), ep_len[i], e.outcome()))
                e.reset()
                ep_rewards[i] = [f32(0.0)] * E.P
                ep_len[i] = 0
        move_counts = [m + 1 for m in move_counts]
        for (i, tot, length, outcome) in done_envs:
            if completed >= num_games:
                continue
            completed += 1
            perm = perms[perm_idx[i]]
            cr = [tot[perm.index(c)] for c in range(ncp)]
            pl = [outcome[perm.index(c)] for c in range(ncp)] if outcome is not None else rewards_to_placements(cr)
            games.append((cr + [f32(0.0)] * (6 - ncp), pl + [0] * (6 - ncp), length, i, perm_idx[i], step))
            for c, place in enumerate(pl):
                if 0 < place <= ncp:
                    placements[c][place - 1] += 1
            move_counts[i] = 0
            perm_idx[i] = (perm_idx[i] + 1) % len(perms)
        remaining = max(0, num_games - completed)
        active = sum(1 for t in terminal if not t)
        if active > remaining:
            to_freeze, frozen = active - remaining, 0
            for (i, _, _, _) in done_envs:
                if frozen >= to_freeze:
                    break
                if not terminal[i]:
                    terminal[i] = True
                    frozen += 1
            for i in range(num_envs):
                if frozen >= to_freeze:
                    break
                if not terminal[i]:
                    terminal[i] = True
                    frozen += 1
        step += 1
    return dict(games=games, rng_pos=int(rng.word_pos), placements=placements, steps=step, ended_by=ended_by,
                max_len=max([g[2] for g in games], default=0))


def games_equal(ref_games, rec):
    """ref_games from run_stats_mode against the device's record array: integers equal,
    f32 rewards equal by bit pattern"""
    if len(ref_games) != len(rec):
        return False
    for (cr, pl, length, env, pi, step), g in zip(ref_games, rec):
        a = np.asarray(cr, f32).view(np.uint32)
        b = np.asarray(g["total_reward"], f32).view(np.uint32)
        if not (np.array_equal(a, b) and list(g["placement"]) == list(pl) and g["length"] == length
                and g["env_index"] == env and g["perm_index"] == pi and g["step"] == step):
            return False
    return True
