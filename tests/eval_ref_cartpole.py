"""CartPole for the Python restatement of stats-mode evaluation (tests/eval_ref.py), and the
cases test_eval_cartpole_ref.py (CPU) and test_gpu_eval_cartpole.py (device) share.  TEST
INFRASTRUCTURE ONLY: the parity checker of bppo_evaluate_episodes.

_CP is the oracle's CartPole (or_cartpole_new / reset / step / get_obs) behind the env interface
of eval_ref: one player, no action mask, no game_outcome.  Registered under "cartpole" in
eval_ref.ENVS, eval_ref.run_stats_mode is the restatement of run_stats_mode_env::<CartPole>
(eval.rs:1621-1877) unchanged; run() adds a trace of which active envs drew a word at each
step."""
import ctypes as C

import numpy as np

import eval_ref as R
import oracle_ffi as O

f32 = np.float32
_get_obs = None


def _cartpole_get_obs():
    global _get_obs
    if _get_obs is None:
        f = O.lib()["or_cartpole_get_obs"]           # a function object of its own: its own argtypes
        f.restype = None
        f.argtypes = [C.POINTER(O.CartPole), C.c_void_p]
        _get_obs = f
    return _get_obs


class _CP:
    D, A, P = 5, 2, 1

    def __init__(self, seed, players):
        self.L = O.lib()
        self.e = O.CartPole()
        self.L.or_cartpole_new(C.byref(self.e), seed)      # CartPole::new resets once (cartpole.rs:104)
        self._obs = np.zeros(self.D, f32)

    def set_num_players(self, n):
        pass

    def reset(self):
        self.L.or_cartpole_reset(C.byref(self.e), self._obs)

    def obs(self):
        _cartpole_get_obs()(C.byref(self.e), self._obs.ctypes.data)
        return self._obs

    def mask(self):
        return None

    def player(self):
        return 0

    def step(self, a):
        r, d = C.c_float(), C.c_int()
        self.L.or_cartpole_step(C.byref(self.e), int(a), self._obs, C.byref(r), C.byref(d))
        return np.array([r.value], f32), bool(d.value)

    def outcome(self):
        return None


R.ENVS["cartpole"] = _CP

_trace = []


class _TracedModel(R.Model):
    """one logits() call per loop iteration (one model): opens the step's draw trace"""

    def logits(self, obs):
        _trace.append([])
        return super().logits(obs)


def run_reference(desc, params, norm, num_envs, num_games, sched, seed, max_steps):
    """run_stats_mode on CartPole with one checkpoint.  The result dict of eval_ref, plus
    draws_per_step [(active envs that drew, active envs that did not)] and draws, their total."""
    orig = R.sample_with_temperature

    def traced(logits, mask, temperature, next_u32):
        a, used = orig(logits, mask, temperature, next_u32)
        _trace[-1].append(used)
        return a, used

    del _trace[:]
    R.sample_with_temperature = traced
    try:
        out = R.run_stats_mode("cartpole", num_envs, 1, [_TracedModel(desc, params, norm)], [0], num_games,
                               R.TempSchedule(*sched), seed, max_steps=max_steps)
    finally:
        R.sample_with_temperature = orig
    out["draws_per_step"] = [(sum(s), len(s) - sum(s)) for s in _trace]
    out["draws"] = sum(d for d, _ in out["draws_per_step"])
    return out


# ------------------------------------------------------------------- cases ---
def net_config(H, NL, act):
    import bppo
    return bppo.make_config("cartpole", hidden_size=H, num_hidden=NL, activation=act, num_envs=8, num_steps=4,
                            num_minibatches=1, num_epochs=1)


def random_net(H, NL, act, seed):
    """orthogonal init x 3: logits of order 0.1 rather than the policy head's 0.01-gain ones, so
    the sampled actions depend on the logits' last bits (as test_gpu_eval.py does)"""
    import bppo
    return (bppo.orthogonal_init(net_config(H, NL, act), seed=seed) * f32(3.0)).astype(f32)


def zero_net(H, NL, act, seed=None):
    import bppo
    return np.zeros_like(bppo.orthogonal_init(net_config(H, NL, act), seed=1))


# the balancing controller: push right iff c . obs >= 0.  c was found with the oracle env
# (test_eval_cartpole_ref.py pins that every episode of the case reaches the 500-step truncation)
BALANCE_C = (0.1, 0.5, 10.0, 2.0, 0.0)
BALANCE_K = 4.0


def balance_net(H, NL, act, seed=None):
    """hidden units 0 and 1 of the first layer carry +(c . obs) and -(c . obs), so with relu
    h0 - h1 = c . obs; a second layer passes the two through; logits = -+K (h0 - h1)"""
    assert act == "relu"
    n = zero_net(H, NL, act).size
    p = np.zeros(n, f32)
    off = 0
    w0 = p[off:off + 5 * H].reshape(5, H); off += 5 * H + H          # [in][out], then b0
    w0[:, 0] = BALANCE_C
    w0[:, 1] = [-c for c in BALANCE_C]
    if NL == 2:
        w1 = p[off:off + H * H].reshape(H, H); off += H * H + H
        w1[0, 0] = w1[1, 1] = 1.0
    wp = p[off:off + 2 * H].reshape(H, 2)
    wp[0] = [-BALANCE_K, BALANCE_K]
    wp[1] = [BALANCE_K, -BALANCE_K]
    return p


def obs_norm(seed, count=500.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=5) * 0.05, (rng.random(5) + 0.5) * 0.02 * count, count)


DEFAULT_TEMP = (0.3, 0.0, None, False)           # the trait's EVAL_TEMP, no cutoff (env.rs:53-58)
# name: hidden, layers, activation, net maker, net seed, normalizer or None, envs, games, schedule, seed
CASES = {
    "default": (64, 2, "relu", random_net, 11, None, 70, 150, DEFAULT_TEMP, 201),
    "greedy": (32, 2, "relu", random_net, 12, None, 70, 150, (0.0, 0.0, None, False), 202),
    "greedy_zero": (32, 2, "relu", zero_net, None, None, 70, 150, (0.0, 0.0, None, False), 203),
    "cutoff": (64, 1, "tanh", random_net, 13, None, 70, 150, (1.0, 0.0, 8, True), 204),
    "normalized": (16, 1, "tanh", random_net, 14, obs_norm(901), 70, 150, DEFAULT_TEMP, 205),
    "normalized_count1": (16, 1, "tanh", random_net, 14, obs_norm(901, 1.0), 70, 150, DEFAULT_TEMP, 205),
    # 11 of the 16 envs are frozen after the first step; the first moves draw, the rest are greedy, so
    # two of the five episodes end at one step
    "freeze": (32, 1, "relu", random_net, 15, None, 16, 5, (0.3, 0.0, 4, False), 207),
    "many_per_thread": (16, 2, "relu", random_net, 16, None, 1100, 1300, DEFAULT_TEMP, 207),
    "truncation": (16, 1, "relu", balance_net, None, None, 8, 10, (0.0, 0.0, None, False), 208),
}
MAX_STEPS = 4000

# pods: per net shape six pods of 48 envs, six different nets, distinct seeds, pod 2 with a normalizer
POD_SHAPES = [(16, 1, "relu"), (16, 2, "tanh"), (32, 1, "tanh"), (32, 2, "tanh"), (64, 1, "relu"), (64, 2, "tanh")]
POD_ENVS, POD_GAMES, N_PODS = 48, 60, 6


def pod_case(shape, k):
    """pod k of a shape as a CASES-style tuple"""
    H, NL, act = shape
    return (H, NL, act, random_net, 300 + 10 * H + NL + 7 * k, obs_norm(950 + k) if k == 2 else None, POD_ENVS,
            POD_GAMES, DEFAULT_TEMP, 4000 + 100 * H + 10 * NL + k)


def case_model(case):
    H, NL, act, make, nseed, norm = case[:6]
    return make(H, NL, act, nseed), norm


_refs = {}


def reference(key, case=None):
    """the restatement of a case, computed once and shared"""
    if key not in _refs:
        case = CASES[key] if case is None else case
        H, NL, act, make, nseed, norm, E, games, sched, seed = case
        params, norm = case_model(case)
        _refs[key] = run_reference(O.mlp_desc(5, 2, H, NL, relu=act == "relu"), params, norm, E, games, sched, seed,
                                   MAX_STEPS)
    return _refs[key]


def pod_reference(shape, k):
    return reference(("pod",) + tuple(shape) + (k,), pod_case(shape, k))
