"""Plain numpy reference of the counter RNG of csrc/spatial.hip (Philox4x32-10) and of the three kernels that draw from it:
dropout_philox (stream word 1), channel_mask_philox (2) and add_noise (3).  No GPU, no torch.

Every function is vectorised over the counters.  The 32-bit words are held in uint64 arrays and masked after each operation, so
that no intermediate depends on numpy's overflow rules.  `u01` is the kernel's own float32 expression (not its comment): the
comparison `u01 > p` of the masks is then exact, and the GPU tests can ask for the reference's pattern bit for bit.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
C3 = 0x9E3779B9                 # the kernels' fixed fourth counter word
STREAM_DROPOUT, STREAM_CHANNEL, STREAM_NOISE = 1, 2, 3
_S32 = np.uint64(32)


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al., Random123).  Counter words c0..c3 and key words k0, k1: scalars or arrays of
    32-bit values (broadcast against each other).  Returns four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) for v in (c0, c1, c2, c3, k0, k1)])
    c0, c1, c2, c3, k0, k1 = (a.copy() for a in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = PHILOX_M0 * c0          # 32 x 32 -> 64 bits: exact in uint64
        p1 = PHILOX_M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n1 = p1 & M32
        n2 = (p0 >> _S32) ^ c3 ^ k1
        n3 = p0 & M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def u01(x):
    """The kernel's uniform: (float32(x >> 8) + 0.5f) * 2^-24, evaluated in float32.  The range is (0, 1]: x >> 8 = 2^24 - 1 gives
    16777215.5, which rounds to 2^24 in float32 (ties to even), hence exactly 1.0."""
    x = np.asarray(x, dtype=np.uint64) & M32
    f = (x >> np.uint64(8)).astype(np.float32)          # < 2^24: exact
    return (f + np.float32(0.5)) * np.float32(2.0 ** -24)


def _words(ngroups, seed, offset, stream):
    """the four output words of counters offset + i, i < ngroups (the 64-bit counter wraps as the kernel's uint64 does)"""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset) + np.arange(ngroups, dtype=np.uint64)
    return philox4x32_10(ctr & M32, ctr >> _S32, stream, C3, seed & 0xFFFFFFFF, seed >> 32)


def _uniforms4(n, seed, offset, stream):
    """(ngroups, 4) float32: u01 of word k of group i at [i, k]"""
    n4 = (int(n) + 3) // 4
    return np.stack([u01(w) for w in _words(n4, seed, offset, stream)], axis=1)


def dropout_keep(n, p, seed, offset):
    """bool (n,): element e = 4 i + k of dropout_philox is kept where u01(word k of counter offset + i) > float32(p)"""
    return (_uniforms4(n, seed, offset, STREAM_DROPOUT) > np.float32(p)).reshape(-1)[:n]


def channel_keep(n, p, seed, offset):
    """bool (n,): entry i of channel_mask_philox is kept where u01(word 0 of counter offset + i) > float32(p)"""
    return u01(_words(int(n), seed, offset, STREAM_CHANNEL)[0]) > np.float32(p)


def noise(n, sigma, clip, seed, offset):
    """float64 (n,): add_noise's draw.  The uniforms are the kernel's float32 values; Box-Muller on the pairs (x, y) and (z, w) of
    each counter (r cos, r sin), the scaling and the clamp are evaluated in float64 (sigma and clip as the float32 values the C ABI
    receives)."""
    sigma, clip = float(np.float32(sigma)), float(np.float32(clip))
    u = _uniforms4(n, seed, offset, STREAM_NOISE).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1).reshape(-1)[:n]
    return np.clip(z * sigma, -clip, clip)
