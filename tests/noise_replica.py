"""The on-device generator of csrc/cld_kernels.h (splitmix64 -> u01 -> Box-Muller, `normal4`) restated in numpy: integer arithmetic in
uint64 with wrap-around and `u01` in float32, both exactly as the kernels compute them; the logarithm, square root, sine and cosine in
float64, so a value differs from the device's float32 `logf` / `sqrtf` / `sincosf` result by their rounding (a few 1e-7) and by nothing
else.  A plain module, imported by tests/test_noise_host.py and tests/test_gpu_noise.py.

Every draw site of the library (head_kernel, the fused updates of conv_chain.hip / chain_wino.hip, the three guidance kernels) keys the
generator by (seed, step, row) with row = b * 52 + l of latent x[b, l, :], step = the iteration index of the sampling loop (0 for the
first, noisiest step) and takes the row's four components as x[b, l, 0..3]: `chain_noise` is that, as the `noise` argument of
Engine.sample."""
import numpy as np

_TWO_PI_F32 = np.float32(6.283185307179586)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def u01(bits):
    """((float)(bits >> 40) + 0.5f) * 2^-24 in float32: the sum rounds to even from 2^23 up, so 1.0 can come out (then log = 0); 0 cannot."""
    return ((bits >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normal4(seed, salt, rows):
    """-> float64 [n, 4]: the four N(0, 1) values of each row (uint32) under (seed, salt), both taken modulo 2^64."""
    rows = np.asarray(rows).reshape(-1).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        ctr = np.uint64((int(salt) << 32) & 0xFFFFFFFFFFFFFFFF) + rows
        k = splitmix64(seed ^ splitmix64(ctr))
        r = [splitmix64(k + np.uint64(j)) for j in range(4)]
    m0 = np.sqrt(-2.0 * np.log(u01(r[0]).astype(np.float64)))
    m1 = np.sqrt(-2.0 * np.log(u01(r[2]).astype(np.float64)))
    a0 = (_TWO_PI_F32 * u01(r[1])).astype(np.float64)       # the product is a float32 one on the device
    a1 = (_TWO_PI_F32 * u01(r[3])).astype(np.float64)
    return np.stack((m0 * np.cos(a0), m0 * np.sin(a0), m1 * np.cos(a1), m1 * np.sin(a1)), axis=-1)


def step_noise(seed, step, B, L=52):
    """-> float64 [B, L, 4]: what iteration `step` of a chain under `seed` draws for a batch of B agents."""
    return normal4(seed, step, np.arange(B * L)).reshape(B, L, 4)


def chain_noise(seed, steps, B, L=52):
    """-> float32 [steps, B, L, 4]: the `noise` argument that makes Engine.sample(noise=...) repeat Engine.sample(noise=None, seed=seed)."""
    return np.stack([step_noise(seed, it, B, L) for it in range(steps)]).astype(np.float32)
