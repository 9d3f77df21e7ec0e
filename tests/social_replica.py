"""The on-device draws of the social-group term (csrc/social_kernels.hip) restated in numpy over tests/noise_replica.py: integer
arithmetic in uint64 with wrap-around and `u01` in float32, exactly as the kernel computes them, so the values are the device's bit
for bit.  For plan row `row` (= agent * num_samp + sample) and step t of the evaluation with index (iteration, optimiser step k):

    e = row * 52 + t,  eval = iteration << 16 | k
    key = splitmix64(seed ^ splitmix64(splitmix64(TAG ^ eval) + e))
    u = u01(splitmix64(key)),  r = (splitmix64(key + 1) >> 32) * (M - 1) >> 32        with M the size of the row's group
"""
import numpy as np

from tests import noise_replica as NR

TAG = 0x536F6369616C4772


def eval_index(iteration, k):
    return ((int(iteration) & 0xFFFFFFFF) << 16) | int(k)


def draws(seed, iteration, k, group_size_of_row, L=52):
    """group_size_of_row [B] (0 for rows outside every group) -> (r int32 [B,L], u float32 [B,L]); rows outside the groups hold r = 0."""
    M = np.asarray(group_size_of_row, dtype=np.uint64).reshape(-1)
    B = M.shape[0]
    e = np.arange(B * L, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = NR.splitmix64(np.uint64(TAG ^ eval_index(iteration, k)))
        key = NR.splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ NR.splitmix64(base + e))
        u = NR.u01(NR.splitmix64(key))
        hi = NR.splitmix64(key + np.uint64(1)) >> np.uint64(32)
        m1 = np.repeat(np.where(M > 0, M - np.uint64(1), np.uint64(0)), L)
        r = (hi * m1) >> np.uint64(32)
    return r.astype(np.int32).reshape(B, L), u.astype(np.float32).reshape(B, L)


def group_size_of_row(groups, A, N):
    """groups (lists of agent indices), A agents, N samples -> [A N] the size of the group of every plan row, 0 outside."""
    size = np.zeros(A, np.int64)
    for g in groups:
        size[np.asarray(g, dtype=np.int64)] = len(g)
    return np.repeat(size, N)
