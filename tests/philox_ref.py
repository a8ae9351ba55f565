"""dgpamd_philox_fill (csrc/philox.hpp, csrc/philox.hip, DESIGN I.23) restated in numpy from the text of include/dgp_amd.h:
Philox4x64-10 on uint64 arrays, the 64 x 64 -> 128 bit products through 32-bit halves, the counter contract, the four kinds, and
twins of the three device stream classes (calibrate.DeviceStreams, calibrate.DeviceSmcStreams, reliability.DeviceSusStreams)
that return numpy arrays in the same layouts.

The contract.  Entry [i, p, r, e] of a (rounds, P, R, D) fill of stream s under key (k0, k1) is word e mod 4 of the block of
the counter c0 = 1 + e div 4, c1 = (p << 32) | r, c2 = c2_first + i, c3 = s: the e-th output of
numpy.random.Philox(counter=[0, c1, c2, c3], key=key).random_raw().  bits: the word; uniform: (w >> 11) 2^-53; log_uniform:
its log; normal: Box and Muller on the pairs of words (0, 1) and (2, 3), u1 = ((w_a >> 11) + 1) 2^-53, u2 = (w_b >> 11) 2^-53,
rho = sqrt(-2 log u1), elements rho cos(2 pi u2) and rho sin(2 pi u2).  The bits and the uniforms are exact; log, cos and sin
here are numpy's, the device's are its own library's, and the GPU test holds both to the exact value of the formula."""
import numpy as np

U = np.uint64
M0, M1 = U(0xD2E7470EE14C6C93), U(0xCA5A826395121157)
W0, W1 = U(0x9E3779B97F4A7C15), U(0xBB67AE8584CAA73B)
ROUNDS = 10
KINDS = ('bits', 'uniform', 'log_uniform', 'normal')
STREAM_PRIOR, STREAM_NORMAL, STREAM_LOGU, STREAM_RESAMPLE = 0, 1, 2, 3
_LOW, _S32 = U(0xFFFFFFFF), U(32)


def key_of(seed):
    """(k0, k1) = numpy.random.SeedSequence(seed).generate_state(2, uint64), as Python integers."""
    k = np.random.SeedSequence(seed).generate_state(2, np.uint64)
    return int(k[0]), int(k[1])


def mulhilo(a, b):
    """(high, low) 64-bit halves of the 128-bit products of the uint64 arrays a and b, through 32-bit halves."""
    a, b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
    a0, a1, b0, b1 = a & _LOW, a >> _S32, b & _LOW, b >> _S32
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1             # (each below 2^64)
    mid = (ll >> _S32) + (lh & _LOW) + (hl & _LOW)                  # (below 3 2^32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32), a * b


def philox(c0, c1, c2, c3, k0, k1):
    """The blocks of the counters (c0, c1, c2, c3), arrays that broadcast, under the key (k0, k1): four uint64 arrays."""
    c = [np.asarray(v, dtype=U) for v in np.broadcast_arrays(*(np.asarray(v, dtype=U) for v in (c0, c1, c2, c3)))]
    k0, k1 = np.asarray(k0, dtype=U), np.asarray(k1, dtype=U)
    with np.errstate(over='ignore'):
        for i in range(ROUNDS):
            if i > 0:
                k0, k1 = k0 + W0, k1 + W1
            hi0, lo0 = mulhilo(M0, c[0])
            hi1, lo1 = mulhilo(M1, c[2])
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def words(key, stream, c2_first, rounds, P, R, D, p0=0, r0=0):
    """(rounds, P, R, D) uint64: the raw words of a fill.  p0, r0: the first path and slot (0 is the device's)."""
    nb = (D + 3) // 4
    i = (np.arange(rounds, dtype=object) + int(c2_first)) % (1 << 64)
    c2 = np.array([int(v) for v in i], dtype=U).reshape(rounds, 1, 1, 1)
    p = (np.arange(P, dtype=U) + U(p0)).reshape(1, P, 1, 1)
    r = (np.arange(R, dtype=U) + U(r0)).reshape(1, 1, R, 1)
    j = np.arange(nb, dtype=U).reshape(1, 1, 1, nb)
    w = philox(U(1) + j, (p << _S32) | r, c2, U(int(stream)), int(key[0]), int(key[1]))
    return np.ascontiguousarray(np.stack(w, -1).reshape(rounds, P, R, 4 * nb)[..., :D])


def to_uniform(w):
    return (w >> U(11)).astype(np.float64) * 2.0 ** -53


def to_uniform_open0(w):
    return ((w >> U(11)) + U(1)).astype(np.float64) * 2.0 ** -53


def normal_uniforms(key, stream, c2_first, rounds, P, R, D):
    """(u1, u2), each (rounds, P, R, ceil(D / 2)): the exactly known uniforms behind elements 2 m and 2 m + 1 of a normal fill,
    rho cos(2 pi u2) and rho sin(2 pi u2) with rho = sqrt(-2 log u1)."""
    w = words(key, stream, c2_first, rounds, P, R, D + D % 2)
    return to_uniform_open0(w[..., 0::2]), to_uniform(w[..., 1::2])


def fill(kind, key, stream, c2_first, rounds, P, R, D, p0=0, r0=0):
    """Engine.philox_fill in numpy: (rounds, P, R, D), int64 for 'bits' and float64 else."""
    if kind not in KINDS:
        raise ValueError('kind')
    Dw = D + D % 2 if kind == 'normal' else D   # (a lone last element needs its pair's second word)
    w = words(key, stream, c2_first, rounds, P, R, Dw, p0, r0)
    if kind == 'bits':
        return w.view(np.int64)
    if kind == 'uniform':
        return to_uniform(w)
    if kind == 'log_uniform':
        with np.errstate(divide='ignore'):
            return np.log(to_uniform(w))
    u1, u2 = to_uniform_open0(w[..., 0::2]), to_uniform(w[..., 1::2])
    rho = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)], -1).reshape(rounds, P, R, Dw)
    return np.ascontiguousarray(z[..., :D])


def stage_round(t, i=0):
    """c2 of move i of stage t."""
    return (int(t) << 32) | int(i)


# ------------------------------------------------------------------------------------------------ the twins of the streams
class Streams:
    """calibrate.DeviceStreams: z of stream 1 (Dx elements) and log u of stream 2 (one element), c2 the iteration."""

    def __init__(self, seed, P, R, Dx):
        self.key, self.P, self.R, self.Dx, self.c = key_of(seed), P, R, Dx, 0

    def block(self, rounds):
        c, self.c = self.c, self.c + rounds
        return (fill('normal', self.key, STREAM_NORMAL, c, rounds, self.P, self.R, self.Dx),
                fill('log_uniform', self.key, STREAM_LOGU, c, rounds, self.P, self.R, 1)[..., 0])


class SmcStreams:
    """calibrate.DeviceSmcStreams: prior uniforms of stream 0 at c2 = 0; per stage t the resampling uniform of stream 3 at
    (c2 = t << 32, r = 0), z of stream 1 and log u of stream 2 (one element) at c2 = (t << 32) | i."""

    def __init__(self, seed, P, R, Dx):
        self.key, self.P, self.R, self.Dx, self.t = key_of(seed), P, R, Dx, 0

    def prior_uniforms(self):
        return fill('uniform', self.key, STREAM_PRIOR, 0, 1, self.P, self.R, self.Dx)[0]

    def stage(self, rounds):
        t, self.t = self.t, self.t + 1
        c2 = stage_round(t)
        return (fill('uniform', self.key, STREAM_RESAMPLE, c2, 1, self.P, 1, 1).reshape(self.P),
                fill('normal', self.key, STREAM_NORMAL, c2, rounds, self.P, self.R, self.Dx),
                fill('log_uniform', self.key, STREAM_LOGU, c2, rounds, self.P, self.R, 1)[..., 0])


class SusStreams:
    """reliability.DeviceSusStreams: prior uniforms of stream 0 at c2 = 0; per stage t z of stream 1 and log u of stream 2,
    Dx elements each, at c2 = (t << 32) | i."""

    def __init__(self, seed, P, R, Dx):
        self.key, self.P, self.R, self.Dx, self.t = key_of(seed), P, R, Dx, 0

    def prior_uniforms(self):
        return fill('uniform', self.key, STREAM_PRIOR, 0, 1, self.P, self.R, self.Dx)[0]

    def stage(self, rounds):
        t, self.t = self.t, self.t + 1
        c2 = stage_round(t)
        return (fill('normal', self.key, STREAM_NORMAL, c2, rounds, self.P, self.R, self.Dx),
                fill('log_uniform', self.key, STREAM_LOGU, c2, rounds, self.P, self.R, self.Dx))
