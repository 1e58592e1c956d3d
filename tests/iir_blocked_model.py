"""The contract of recursive filtering parallel in time (include/grail_hip.h, "levels, continued: recursive filtering,
parallel in time") in numpy, on top of iir_model's clean, table, run and to_f32: the blocks of all rows are the rows of `run`
(the rest pass, then the output pass from the entry states), T is `run` on zeros from the unit states, and the entry states
are a Python loop over blocks in the header's order: ascending j up to the state's own section, one product and one addition
each (Python's float is binary64, every operation rounded by itself), z added last."""
import numpy as np

from iir_model import REFUSED, SECTIONS_MAX, clean, run, table, to_f32

BLOCK = 1024


def block_matrix(coef, block=BLOCK):
    """T float64 [2 S][2 S] of one filter (float64 [S][5] or flat): T[i][c] = state i (s1[0] s2[0] s1[1] ...) after `block`
    steps on +0.0 input from the state that is 1.0 in place c"""
    c, S = table([coef], [0])
    n = 2 * int(S[0])
    c, S = np.repeat(c, n, 0), np.repeat(S, n)
    s1, s2 = np.zeros((n, SECTIONS_MAX)), np.zeros((n, SECTIONS_MAX))
    for col in range(n):
        (s2 if col & 1 else s1)[col, col // 2] = 1.0
    run(np.zeros((n, block)), np.full(n, block), c, S, s1, s2)
    T = np.zeros((n, n))
    T[0::2] = s1[:, :n // 2].T
    T[1::2] = s2[:, :n // 2].T
    return T


def entry_states(T, z):
    """z float64 [K - 1][2 S], the rest pass's end states -> e float64 [K][2 S], the blocks' entry states"""
    n = T.shape[0]
    Tl = T.tolist()
    e = [[0.0] * n]
    with np.errstate(all="ignore"):
        for zk in z.tolist():
            ek, nxt = e[-1], []
            for i in range(n):
                acc = Tl[i][0] * ek[0]
                for j in range(1, 2 * (i // 2) + 2):
                    acc = acc + Tl[i][j] * ek[j]
                nxt.append(acc + zk[i])
            e.append(nxt)
    return np.array(e, np.float64).reshape(-1, n)


def iir_blocked_model(rows, filters, which=None, tail=0, out_stride=None, lens=None, exact=False, block=BLOCK):
    """grail_biquad_blocked_async, with iir_model's arguments and results: a list of (out float32 [n_out], n_out, nonfinite), or
    (None, REFUSED, 0) for a row whose index is outside the set."""
    which = [0] * len(rows) if which is None else list(which)
    result = [(None, REFUSED, 0)] * len(rows)
    ok = [r for r in range(len(rows)) if which[r] < len(filters)]
    vs, owner, first, facts = [], [], {}, {}
    for r in ok:
        x = np.asarray(rows[r], np.float32)[:None if lens is None else min(int(lens[r]), len(rows[r]))]
        n = len(x)
        n_out = 0 if n == 0 else n + tail
        if out_stride is not None:
            n_out = min(n_out, out_stride)
        steps = max(n, n_out)
        K = -(-steps // block)
        vx, bad = clean(x)                                      # (over all n samples, also where out_stride cut the output)
        v = np.zeros(K * block)
        v[:n] = vx
        first[r], facts[r] = len(owner), (n_out, bad, steps, K)
        vs.append(v.reshape(K, block))
        owner += [r] * K
    if not owner:
        for r in ok:
            result[r] = (np.zeros(0, np.float64 if exact else np.float32), 0, facts[r][1])
        return result
    v = np.concatenate(vs)
    c, S = table(filters, [which[r] for r in owner])
    # the rest pass: every block that is not its row's last, from rest over its B inputs
    inner = np.array([i for i, r in enumerate(owner) if i - first[r] < facts[r][3] - 1], np.int64)
    z1, z2 = np.zeros((len(inner), SECTIONS_MAX)), np.zeros((len(inner), SECTIONS_MAX))
    if len(inner):
        run(v[inner], np.full(len(inner), block), c[inner], S[inner], z1, z2)
    at = {int(i): k for k, i in enumerate(inner)}
    # the entry states, row by row
    s1, s2 = np.zeros((len(owner), SECTIONS_MAX)), np.zeros((len(owner), SECTIONS_MAX))
    steps_of = np.zeros(len(owner), np.int64)
    matrices = {}
    for r in ok:
        n_out, bad, steps, K = facts[r]
        f, i0 = which[r], first[r]
        steps_of[i0:i0 + K] = np.minimum(block, steps - block * np.arange(K))
        if K < 2:
            continue
        if f not in matrices:
            matrices[f] = block_matrix(filters[f], block)
        Sf = matrices[f].shape[0] // 2
        z = np.zeros((K - 1, 2 * Sf))
        for k in range(K - 1):
            z[k, 0::2], z[k, 1::2] = z1[at[i0 + k], :Sf], z2[at[i0 + k], :Sf]
        e = entry_states(matrices[f], z)
        s1[i0:i0 + K, :Sf], s2[i0:i0 + K, :Sf] = e[:, 0::2], e[:, 1::2]
    # the output pass: every block from its entry state over its own steps
    y = run(v, steps_of, c, S, s1, s2)
    for r in ok:
        n_out, bad, steps, K = facts[r]
        yr = y[first[r]:first[r] + K].reshape(-1)[:n_out]
        result[r] = (yr.copy() if exact else to_f32(yr), n_out, bad)
    return result
