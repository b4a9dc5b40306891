"""A host model of csrc/drop_hash.hpp in numpy, and the index every kernel that draws a dropout mask hashes.  No GPU, no library import.

The functions of the first half are the header's, word for word, on uint32 / uint64 arrays (tests/test_dropout_reference_cpu.py compiles the
header into a host program and holds this model to it bit for bit, then checks the model's statistics).  The second half is one function per
dropout site, each returning the boolean KEEP mask of that site; the index expressions are read off the kernels (file and line beside each),
not inferred from outputs.  The GPU sweeps compare every mask the device draws with these, bit for bit: a kernel that hashes another index,
a tile that re-derives another group's word, or a change of the hash itself (which would change the masks of every checkpointed run) fails
them.
"""
import numpy as np

U32 = np.uint32
U64 = np.uint64
GOLD = 0x9E3779B9
MURM = 0x85EBCA6B
DEFAULT_SEED = 1234          # runtime.Context.init_device(seed=1234)


def _u32(x):
    """any integer array / scalar -> uint32 array, modulo 2^32 (the C cast)"""
    return (np.asarray(x).astype(U64) & U64(0xFFFFFFFF)).astype(U32)


def _mul(x, k):
    """uint32 * constant modulo 2^32, through uint64 (no overflow warnings)"""
    return ((np.asarray(x).astype(U64) * U64(k)) & U64(0xFFFFFFFF)).astype(U32)


def _add(*xs):
    s = np.zeros((), U64)
    for x in xs:
        s = s + np.asarray(x).astype(U64)
    return (s & U64(0xFFFFFFFF)).astype(U32)


def _lo(x):
    return _u32(np.asarray(x, dtype=U64))


def _hi(x):
    return (np.asarray(x, dtype=U64) >> U64(32)).astype(U32)


def mix32(x):
    x = _u32(x)
    x = x ^ (x >> U32(16))
    x = _mul(x, 0x7feb352d)
    x = x ^ (x >> U32(15))
    x = _mul(x, 0x846ca68b)
    return x ^ (x >> U32(16))


def uniform01(seed, salt, idx):
    """float32 in [0, 1): (h >> 8) * 2^-24, exact"""
    seed, idx = np.asarray(seed, dtype=U64), np.asarray(idx, dtype=U64)
    a = mix32(_lo(idx) ^ _lo(seed))
    b = mix32(_hi(idx) ^ _hi(seed) ^ _mul(_u32(salt), GOLD))
    h = mix32(a ^ _add(b, GOLD, a << U32(6), a >> U32(2)))
    return ((h >> U32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def drop_quad(seed, salt, quad):
    """-> (h0, h1), the two words of a quad of the flat index (quad is 64 bits wide)"""
    seed, quad = np.asarray(seed, dtype=U64), np.asarray(quad, dtype=U64)
    h0 = mix32(_add(_lo(quad) ^ _lo(seed), _mul(_u32(salt), GOLD)))
    h1 = mix32(h0 ^ _hi(quad) ^ _hi(seed) ^ _mul(_u32(salt), MURM))
    return h0, h1


def drop_words8(seed, salt, group):
    """-> (h0, h1, h2, h3), the four words of a group of 8 channels (group is 32 bits wide: the kernel's index arithmetic is unsigned)"""
    seed = np.asarray(seed, dtype=U64)
    h0 = mix32(_add(_u32(group) ^ _lo(seed), _mul(_u32(salt), GOLD)))
    h1 = mix32(h0 ^ _hi(seed) ^ _mul(_u32(salt), MURM))
    h2 = mix32(_add(h1, GOLD, h0 << U32(6)))
    h3 = mix32(h2 ^ U32(MURM) ^ (h1 >> U32(2)))
    return h0, h1, h2, h3


def mha_drop4(seed, salt, group):
    """-> (h0, h1): drop_words8's first two words"""
    return drop_words8(seed, salt, group)[:2]


def drop_thr16(p):
    """uint32(float32(p) * float32(65536)): the product is exact (a power of two), the cast truncates"""
    return U32(int(np.float32(p) * np.float32(65536.0)))


def lane16(words, e):
    """the 16-bit uniform of element e of a group: drop_quad_keep / drop_keep8 / mha_keep4 compare this with the threshold.
    words: tuple of uint32 arrays, e: integer array broadcastable to them (0 <= e < 2 len(words))"""
    e = np.asarray(e)
    w = np.stack(np.broadcast_arrays(*words), 0)
    picked = np.take_along_axis(w, np.broadcast_to(e >> 1, w.shape[1:])[None].astype(np.intp), 0)[0]
    return (picked >> (U32(16) * (e & 1).astype(U32))) & U32(0xFFFF)


def keep16(words, e, thr):
    return lane16(words, e) >= U32(thr)


def p_eff(p):
    """the drop probability the 16-bit threshold really gives"""
    return int(drop_thr16(p)) / 65536.0


def keep_scale(p):
    """ks = 1.f / (1.f - p) as the kernels form it, in float32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def context_seed(seed=DEFAULT_SEED):
    """the seed word runtime.Context.init_device puts on the device"""
    return seed * 0x9E3779B97F4A7C15 % (1 << 63)


# ---------------------------------------------------------------------------------------------------------------------------------
# one function per site -> boolean KEEP mask
# ---------------------------------------------------------------------------------------------------------------------------------
def element_mask(seed, salt, p, n):
    """emrt_dropout_fwd / emrt_mask_bwd, mode 0 (elementwise.hip: drop_quad(sd, salt, i) with i the quad of the flat index) -> [n]"""
    h0, h1 = drop_quad(seed, salt, np.arange((n + 3) // 4, dtype=U64))          # one draw per quad, its four lanes side by side
    lanes = np.stack([h0 & U32(0xFFFF), h0 >> U32(16), h1 & U32(0xFFFF), h1 >> U32(16)], 1).reshape(-1)[:n]
    return lanes >= drop_thr16(p)


def channel_mask(seed, salt, p, n, hw, C):
    """emrt_dropout_fwd / emrt_mask_bwd, mode 1 (Dropout2D on NHWC rows of C): uniform01 at (idx / C / hw) * C + idx % C, >= p in float32"""
    idx = np.arange(n, dtype=np.int64)
    return uniform01(seed, salt, ((idx // C // hw) * C + idx % C).astype(U64)) >= np.float32(p)


def layernorm_mask(seed, salt, p, rows, C):
    """emrt_layernorm_fwd / _bwd with a fused branch dropout (norm.hip: drop_quad at (row * C + c) >> 2, forward and backward) -> [rows, C]"""
    return element_mask(seed, salt, p, rows * C).reshape(rows, C)


def conv_drop_mask(seed, salt, p, M, OC):
    """emrt_conv2d_drop (conv.hip: drop_words8 at (m * OC + n0) >> 3, n0 the first channel of the group of 8; OC % 8 == 0) -> [M, OC]"""
    m, n = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(OC, dtype=np.int64), indexing="ij")
    n0 = n & ~np.int64(7)
    return keep16(drop_words8(seed, salt, _u32((m * OC + n0) >> 3)), n & 7, drop_thr16(p))


def mha_mfma_mask(seed, salt, p, B, M, L):
    """the MFMA attention kernels (attn.hip: mha_drop4 at ((b * M + m) * L + i) * 32 + (j >> 2), element j & 3) -> [B, M, L(i), L(j)]"""
    bm, i, j = np.meshgrid(np.arange(B * M, dtype=np.int64), np.arange(L, dtype=np.int64), np.arange(L, dtype=np.int64), indexing="ij")
    return keep16(mha_drop4(seed, salt, _u32((bm * L + i) * 32 + (j >> 2))), j & 3, drop_thr16(p)).reshape(B, M, L, L)


def mha_valu_mask(seed, salt, p, B, M, L):
    """the VALU attention kernels (attn.hip: uniform01 at ((b * M + m) * L + i) * L + j, >= pdrop in float32; the backward's loops run over the
    transposed pair but form the same index) -> [B, M, L(i), L(j)]"""
    idx = np.arange(B * M * L * L, dtype=np.int64)
    return (uniform01(seed, salt, idx.astype(U64)) >= np.float32(p)).reshape(B, M, L, L)
