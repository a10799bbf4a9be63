"""The reference model of the ensemble noise (include/fluid_amd.h, "ensemble noise"), in numpy, shared by
tests/test_noise_abi.py (CPU) and tests/test_gpu_noise.py (GPU).  Philox4x32-10 on uint64 arrays -- a 32 x 32 -> 64 product
fits one --, S as an integer, z and the SET / ADD rules in float64: numpy's double operations are IEEE and unfused, so
every line below is one rounding, in the order the header gives."""
import numpy as np

from relax_model import narrow

F32 = np.float32
F64 = np.float64
U64 = np.uint64

M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = U64(0x9E3779B9), U64(0xBB67AE85)
MASK = U64(0xFFFFFFFF)
SH32, SH16 = U64(32), U64(16)
C = float.fromhex("0x1.3988e1412ed76p-16")
DENSE_TAG = 15
SET, ADD = 0, 1

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def _u(a):
    return np.asarray(a).astype(U64) & MASK


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: the four output words (uint64 arrays holding 32-bit values) of counter (c0 .. c3) under key (k0, k1);
    the arguments broadcast against each other."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_u(c0), _u(c1), _u(c2), _u(c3), _u(k0), _u(k1))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> SH32) ^ c1 ^ k0, p1 & MASK, (p0 >> SH32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def halves_sum(words):
    """S: the sum of the eight 16-bit halves of the four words, int64 in [0, 524280]"""
    s = np.zeros(np.shape(words[0]), np.int64)
    for w in words:
        s = s + (w & U64(0xFFFF)).astype(np.int64) + (w >> SH16).astype(np.int64)
    return s


def z_of(seed, sequence, tag, ident, c0, c1):
    """z of the counter (c0, c1, (tag << 16) | ident, sequence) under the 64-bit `seed`: float64, one rounding"""
    seed = int(seed)
    word2 = (np.asarray(tag).astype(U64) << SH16) | np.asarray(ident).astype(U64)
    s = halves_sum(philox(c0, c1, word2, sequence, seed & 0xFFFFFFFF, seed >> 32))
    return (s - 262140).astype(F64) * F64(C)


def field_z(w, members, seed, sequence, field, member_offset=0):
    """(members, w, w) float64: z of every cell (row i, column j) of every member of a field"""
    m = np.arange(members).reshape(-1, 1, 1) + member_offset
    i = np.arange(w).reshape(1, -1, 1)
    j = np.arange(w).reshape(1, 1, -1)
    return z_of(seed, sequence, field, m, j, i)


def amplitudes(amplitude, members):
    a = np.asarray(amplitude, F32)
    return (np.full(members, a, F32) if a.ndim == 0 else a).astype(F64).reshape(-1, 1, 1)


def noise_set(w, members, amplitude, seed, sequence, field, storage=0, member_offset=0):
    """FLUID_NOISE_SET: what the pack shows afterwards, (members, w, w) float32"""
    z = field_z(w, members, seed, sequence, field, member_offset)
    return narrow((amplitudes(amplitude, members) * z).astype(F32), storage)


def noise_add(x, amplitude, seed, sequence, field, storage=0, member_offset=0):
    """FLUID_NOISE_ADD on what the pack shows, x: (members, w, w) float32.  A member whose amplitude is +-0 keeps every
    bit."""
    x = np.asarray(x, F32)
    members, w = x.shape[0], x.shape[1]
    a = amplitudes(amplitude, members)
    with np.errstate(all="ignore"):
        p = a * field_z(w, members, seed, sequence, field, member_offset)
        y = narrow((x.astype(F64) + p).astype(F32), storage)
    return np.where(a != 0, y, x)


def noise_dense(count, amplitude, seed, sequence, stream_id, first=0):
    """fluid_noise_dense: out[first .. first + count), float32"""
    q = np.arange(first, first + count, dtype=U64)
    z = z_of(seed, sequence, DENSE_TAG, stream_id, q & MASK, q >> SH32)
    return (F64(F32(amplitude)) * z).astype(F32)
