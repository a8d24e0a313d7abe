"""Host model of the samplers' in-kernel noise generator (philox_cnormal, sgmse_amd/csrc/kernels_attn_misc.h), in NumPy.

One complex standard normal (Re, Im ~ N(0, 1/2)) per (seed, stream id, element index inside the utterance, draw):

    counter = (idx.lo,  idx.hi ^ stream.lo * 0x9E3779B9,  draw,  0x5367534D ^ stream.lo)
    key     = (seed.lo ^ stream.hi * 0x85EBCA6B,  seed.hi ^ stream.hi)
    (c0, c1, ..) = Philox4x32-10(counter, key)
    u1 = ((c0 >> 8) + 0.5) / 2^24,  u2 = ((c1 >> 8) + 0.5) / 2^24
    z  = sqrt(-ln u1) * (cos 2 pi u2 + i sin 2 pi u2)

Two flavours: ``cnormal64`` evaluates the last three lines in float64 (the reference of the tests), ``cnormal32`` in float32 in the
kernel's own expression order (the deviation between the two is what fp32 costs; the tests take their bounds from it).

The draw schedule of the samplers (engine.h: pc_sample, sb_sample, draw_prior), which ``pc_draws`` / ``replay`` restate:
prior = draw 0; PC step s, corrector pass cs = 1 + cs + s * (ncorr + pred_noise); its predictor = 1 + ncorr + s * (ncorr + pred_noise);
Schroedinger-bridge step s = draw s."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (Weyl sequence)
MASK32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al. 2011, Random123).  ctr: four uint32 arrays (or scalars), key: two.  Returns four
    uint32 arrays.  The key is bumped after every round, as the kernel does."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in key)
    m32, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & m32, (p0 >> sh) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return [v.astype(np.uint32) for v in c]


def counter_words(seed, idx, draw, stream=0):
    """(counter, key) of one draw, as philox_cnormal lays them out.  seed, stream: Python ints below 2^64; idx: integer array."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    slo, shi = stream & MASK32, stream >> 32
    idx = np.asarray(idx, dtype=np.uint64)
    c0 = idx & np.uint64(MASK32)
    c1 = (idx >> np.uint64(32)) ^ np.uint64((slo * W0) & MASK32)
    c2 = np.full(idx.shape, int(draw) & MASK32, dtype=np.uint64)
    c3 = np.full(idx.shape, 0x5367534D ^ slo, dtype=np.uint64)
    k0 = (seed & MASK32) ^ ((shi * 0x85EBCA6B) & MASK32)
    k1 = (seed >> 32) ^ shi
    return (c0, c1, c2, c3), (k0, k1)


def box_muller64(k1, k2):
    """float64: the 24-bit integers k1, k2 -> complex128."""
    u1 = (np.asarray(k1, dtype=np.float64) + 0.5) / 16777216.0
    u2 = (np.asarray(k2, dtype=np.float64) + 0.5) / 16777216.0
    rad = np.sqrt(-np.log(u1))
    ang = 2.0 * np.pi * u2
    return rad * np.cos(ang) + 1j * (rad * np.sin(ang))


def box_muller32(k1, k2):
    """float32 in the kernel's expression order -- ((float)k + 0.5f) * (1.0f / 16777216.0f); sqrtf(-logf(u1));
    sincosf(6.283185307179586f * u2) -- -> complex64."""
    f = np.float32
    u1 = (np.asarray(k1).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    u2 = (np.asarray(k2).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    rad = np.sqrt(-np.log(u1))
    ang = f(6.283185307179586) * u2
    assert rad.dtype == np.float32 and ang.dtype == np.float32
    out = np.empty(rad.shape, dtype=np.complex64)
    out.real, out.imag = rad * np.cos(ang), rad * np.sin(ang)
    return out


def _bits(seed, idx, draw, stream):
    ctr, key = counter_words(seed, idx, draw, stream)
    c = philox4x32_10(ctr, key)
    return c[0] >> np.uint32(8), c[1] >> np.uint32(8)


def cnormal64(seed, idx, draw, stream=0):
    return box_muller64(*_bits(seed, idx, draw, stream))


def cnormal32(seed, idx, draw, stream=0):
    return box_muller32(*_bits(seed, idx, draw, stream))


def replay(seed, streams, per, draws, flavour=cnormal32):
    """The noise of len(draws) draws of a uniform batch as the replayed-noise path reads it: [len(draws), B, per], utterance b on
    stream streams[b], the element index running inside the utterance."""
    idx = np.arange(per)
    return np.stack([np.stack([flavour(seed, idx, d, s) for s in streams]) for d in draws])


def pc_draws(N, ncorr, pred_noise):
    """The draw indices a PC run consumes, in the order of the reference's randn_like calls: prior, then per step the corrector
    passes and the predictor."""
    per_step = ncorr + (1 if pred_noise else 0)
    order = [0]
    for s in range(N):
        order += [1 + cs + s * per_step for cs in range(ncorr)]
        if pred_noise:
            order.append(1 + ncorr + s * per_step)
    return order
