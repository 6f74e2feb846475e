"""tests/ret_norm_ref.py (the plain f64 restatement the device's return-normalizer kernels are
compared with) against the oracle's or_ret_norm_update_return / update_variance / normalize /
reset_player, driven element by element as oracle/ppo.c:376-383 drives them: bit for bit, for
P = 1, 2, 4, 5, 6 on the input families of tests/test_gpu_return_norm.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_ffi as O
from ret_norm_ref import fresh_state, make_inputs, return_norm_ref, seeded_state


def _oracle(gamma, clip, inp, R0, stats3):
    """the oracle's calls in the rollout's order -> (rew, returns [N, P], (mean, m2, count), all_rewards)"""
    rew_raw, done, players, valid = inp["rew_raw"], inp["done"], inp["players"], inp["valid"]
    T, N = rew_raw.shape
    P = R0.shape[1]
    L = O.lib()
    n = O.RetNorm()
    L.or_ret_norm_init(C.byref(n), N, P, gamma, clip)
    for i, x in enumerate(R0.reshape(-1)):
        n.returns[i] = x
    n.mean, n.var, n.count = (float(x) for x in stats3)
    rew = np.zeros((T, N), np.float32)
    allr = inp["all_rewards"].copy()
    ref = C.byref(n)
    for t in range(T):
        for e in range(N):
            p = int(players[t, e])
            r = float(rew_raw[t, e])
            L.or_ret_norm_update_return(ref, e, p, r)
            if valid is None or valid[t, e] > 0.5:
                L.or_ret_norm_update_variance(ref, e, p)
            z = L.or_ret_norm_normalize(ref, r)
            if done[t, e] != 0:
                L.or_ret_norm_reset_player(ref, e, p)
            rew[t, e] = z
            allr[t, e, p] = z
    R = np.array([n.returns[i] for i in range(N * P)]).reshape(N, P)
    out = rew, R, np.array([n.mean, n.var, n.count]), allr
    L.or_ret_norm_free(ref)
    return out


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


FAMILIES = [  # rewards, dones, valid, seeded, clip
    ("sparse", "random", None, False, 10.0),
    ("dense", "step", None, True, 10.0),
    ("sparse", "none", "random", True, 10.0),
    ("dense", "random", "done", False, 10.0),
    ("sparse", "step", "head", False, 10.0),
    ("dense", "random", "none", True, 10.0),
    ("dense", "random", "random", True, 0.5),
]


@pytest.mark.parametrize("P", [1, 2, 4, 5, 6])
@pytest.mark.parametrize("rewards,dones,valid,seeded,clip", FAMILIES)
def test_restatement_equals_oracle_bit_for_bit(P, rewards, dones, valid, seeded, clip):
    T, N = 17, 23
    inp = make_inputs(100 * P + len(rewards) + len(dones), T, N, P, rewards, dones, valid, head=150)
    R0, st0 = seeded_state(P, N, P) if seeded else fresh_state(N, P)
    ref = return_norm_ref(0.99, clip, inp["rew_raw"], inp["done"], inp["players"], inp["valid"], R0, st0,
                          inp["all_rewards"])
    rew, R, st, allr = _oracle(0.99, clip, inp, R0, st0)
    assert np.array_equal(_bits32(ref["rew"]), _bits32(rew))
    assert np.array_equal(_bits64(ref["returns_state"]), _bits64(R))
    assert np.array_equal(_bits64(ref["stats3"]), _bits64(st))
    assert np.array_equal(_bits32(ref["all_rewards"]), _bits32(allr))
    # the restatement's own bookkeeping, and the family does what its name says
    raw = ~ref["normalized"]
    assert np.array_equal(_bits32(ref["rew"][raw]), _bits32(inp["rew_raw"][raw]))
    if not seeded and valid is None:
        assert raw.sum() == 1                      # only the very first element sees n < 2
    if valid == "head":
        assert raw.reshape(-1)[:151].all() and not raw.reshape(-1)[151:].any()
    if valid == "none":
        assert np.array_equal(_bits64(st), _bits64(st0))
    if clip == 0.5:
        c = ref["clamped"]
        assert (c == 1).any() and (c == -1).any() and (c == 0).sum() > c.size // 10
    if P > 1:                                      # every player's return moved
        assert (ref["returns_state"] != R0).any(axis=0).all()


def test_players_none_is_player_zero():
    inp = make_inputs(3, 9, 11, 1, "dense", "random")
    assert not inp["players"].any()
    R0, st0 = seeded_state(3, 11, 1)
    a = return_norm_ref(0.99, 10.0, inp["rew_raw"], inp["done"], None, None, R0, st0)
    b = return_norm_ref(0.99, 10.0, inp["rew_raw"], inp["done"], inp["players"], None, R0, st0)
    assert np.array_equal(_bits32(a["rew"]), _bits32(b["rew"]))
    assert np.array_equal(_bits64(a["returns_state"]), _bits64(b["returns_state"]))
    assert np.array_equal(_bits64(a["stats3"]), _bits64(b["stats3"]))
