"""The ReturnNormalizer's per-step order, restated plainly in f64 (normalization.rs:156-197 as
ppo.rs:388-428 calls it; the oracle's or_ret_norm_* in oracle/vecenv.c, driven as
oracle/ppo.c:376-383 drives them).  No device, no scan: one element after the other.

tests/test_ret_norm_ref.py ties this file to the oracle bit for bit; the device kernels are
compared with it in tests/test_gpu_return_norm.py.

TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

EPS = 1e-8


def return_norm_ref(gamma, clip, rew_raw, done, players, valid, returns_state, stats3, all_rewards=None):
    """rew_raw, done [T, N] f32; players [T, N] i32 or None (player 0 acts everywhere); valid
    [T, N] f32 or None; returns_state [N, P] f64; stats3 = (mean, m2, count); all_rewards
    [T, N, P] f32 or None.  Nothing is modified.  ->
    dict(rew [T, N] f32, returns_state [N, P], stats3 [3], all_rewards or None,
         normalized [T, N] bool: the element left through the n >= 2 branch,
         clamped [T, N] int8: -1 / +1 where the lower / upper clamp engaged)"""
    rew_raw = np.asarray(rew_raw, np.float32)
    T, N = rew_raw.shape
    R = np.array(returns_state, np.float64).reshape(N, -1).copy()
    mean, m2, n = (float(x) for x in stats3)
    gamma = float(gamma)
    clip = np.float32(clip)
    rew = np.zeros((T, N), np.float32)
    normalized = np.zeros((T, N), bool)
    clamped = np.zeros((T, N), np.int8)
    allr = None if all_rewards is None else np.array(all_rewards, np.float32).reshape(T, N, -1).copy()
    for t in range(T):
        for e in range(N):
            p = 0 if players is None else int(players[t, e])
            r = rew_raw[t, e]
            x = float(R[e, p]) * gamma + float(r)                # 1. update_return
            R[e, p] = x
            if valid is None or valid[t, e] > 0.5:               # 2. update_variance (Welford)
                n += 1.0
                delta = x - mean
                mean += delta / n
                m2 += delta * (x - mean)
            z = r                                                # 3. normalize
            if n >= 2.0:
                z = np.float32(float(r) / math.sqrt(m2 / n + EPS))
                normalized[t, e] = True
                if z < -clip:
                    z, clamped[t, e] = -clip, -1
                if z > clip:
                    z, clamped[t, e] = clip, 1
            rew[t, e] = z
            if done[t, e] != 0:                                  # 4. reset_player, valid or not
                R[e, p] = 0.0
            if allr is not None:                                 # 5. the acting player's slot
                allr[t, e, p] = z
    return dict(rew=rew, returns_state=R, stats3=np.array([mean, m2, n]), all_rewards=allr,
                normalized=normalized, clamped=clamped)


# ------------------------------------------------------------- input families ---
SPARSE = np.array([1.0, -1.0, 0.33, -0.33, 0.0], np.float32)     # what Skull and Liar's Dice pay


def make_inputs(seed, T, N, P, rewards="sparse", dones="random", valid=None, head=0):
    """-> dict(rew_raw, done, players, valid, all_rewards): one draw of a family.
    rewards: "sparse" ({+-1, +-0.33, 0}, mostly 0) | "dense" (normal);
    dones: "random" (about 5 %) | "step" (the same, plus one step on which every env ends) | "none";
    valid: None | "random" (about half) | "head" (the first `head` rows in (t, e) order invalid)
    | "none" (all invalid) | "done" (every done row invalid, and a tenth of the others)."""
    rng = np.random.default_rng(seed)
    if rewards == "sparse":
        rew = SPARSE[rng.choice(5, size=(T, N), p=[0.12, 0.08, 0.1, 0.1, 0.6])]
    else:
        rew = (rng.standard_normal((T, N)) * 0.7 + 0.1).astype(np.float32)
    done = np.zeros((T, N), np.float32)
    if dones != "none":
        done[rng.random((T, N)) < 0.05] = 1.0
        if dones == "step":
            done[T // 2] = 1.0
    players = rng.integers(0, P, (T, N)).astype(np.int32)
    if valid is None:
        v = None
    elif valid == "random":
        v = (rng.random((T, N)) < 0.5).astype(np.float32)
    elif valid == "head":
        v = np.ones(T * N, np.float32)
        v[:head] = 0.0
        v = v.reshape(T, N)
    elif valid == "none":
        v = np.zeros((T, N), np.float32)
    elif valid == "done":
        v = (rng.random((T, N)) < 0.9).astype(np.float32)
        v[done != 0] = 0.0
    else:
        raise ValueError(valid)
    # all_rewards: every player's raw reward of the step; the acting player's is rew_raw
    allr = (rng.standard_normal((T, N, P)) * 0.5).astype(np.float32)
    np.put_along_axis(allr, players[..., None].astype(np.int64), rew[..., None], axis=2)
    return dict(rew_raw=np.ascontiguousarray(rew, np.float32), done=done, players=players, valid=v,
                all_rewards=allr)


def seeded_state(seed, N, P):
    """statistics with history and a non-zero rolling return in every one of the N x P slots"""
    rng = np.random.default_rng(seed + 9001)
    R = rng.standard_normal((N, P)) * 0.8
    R[np.abs(R) < 0.05] = 0.5
    return R, np.array([0.07, 640.0 * 0.9, 640.0])


def fresh_state(N, P):
    return np.zeros((N, P)), np.zeros(3)
