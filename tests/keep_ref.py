"""The dropout keep-bit stream of vqa_dropout_mask, restated in NumPy uint64 arithmetic (csrc/vqa_common.h: mix64,
keep_thr, keep_bit): bit i of a site is a function of (seed, offset + i) alone.

  key   = mix64(seed)
  r(p)  = mix64(key ^ (p >> 2))               one 64-bit hash per aligned group of four positions
  u(p)  = (r(p) >> 16 (p & 3)) & 0xFFFF       the group's four 16-bit uniforms
  bit   = u(p) < floor(keep * 65536)          (clamped to 0 .. 65536)
"""
import numpy as np

U64 = np.uint64


def mix64(z):
    """splitmix64 finaliser, element-wise on uint64 (wrapping arithmetic)"""
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def keep_thr(keep):
    t = float(np.float32(keep) * np.float32(65536.0))
    return 0 if t <= 0.0 else (65536 if t >= 65536.0 else int(t))


def keep_bits(n, seed, offset, keep):
    """uint8 [n]: what vqa_dropout_mask(out, n, seed, offset, keep) writes"""
    key = mix64(U64(seed))
    with np.errstate(over="ignore"):
        pos = U64(offset) + np.arange(n, dtype=U64)
    r = mix64(key ^ (pos >> U64(2)))
    u = (r >> (U64(16) * (pos & U64(3)))) & U64(0xFFFF)
    return (u < U64(keep_thr(keep))).astype(np.uint8)
