// The counter-based hashes behind every dropout mask, shared by every kernel that draws one: emrt_dropout_fwd / emrt_mask_bwd (elementwise.hip),
// the LayerNorm kernels with a fused branch dropout (norm.hip), emrt_conv2d_drop (conv.hip) and the emrt_mha_* kernels (attn.hip).  One text, so
// the kernels cannot drift apart -- and, because it includes nothing from HIP, a plain host compiler reads the same text: the suite compiles it
// into a host program and holds tests/dropout_reference.py (the numpy model the GPU tests compare every mask with) to it bit for bit.
// A change here changes the masks of every checkpointed run.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EMRT_DROP_FN __host__ __device__ __forceinline__
#else
#define EMRT_DROP_FN inline
#endif

namespace emrt {

// counter-based RNG for dropout: one 32-bit hash of (seed, salt, index).  keep iff u >= p.
EMRT_DROP_FN uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
EMRT_DROP_FN float uniform01(uint64_t seed, uint32_t salt, uint64_t idx) {
  uint32_t a = mix32((uint32_t)idx ^ (uint32_t)seed);
  uint32_t b = mix32((uint32_t)(idx >> 32) ^ (uint32_t)(seed >> 32) ^ (salt * 0x9E3779B9U));
  uint32_t h = mix32(a ^ (b + 0x9E3779B9U + (a << 6) + (a >> 2)));
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// Element-mode dropout (nn.Dropout on token tensors: the stand-alone kernels and the LayerNorm kernels that apply a branch's dropout themselves):
// the kernels move 4 consecutive elements per lane, so ONE 64-bit draw per aligned quad of the flat index gives their four 16-bit uniforms --
// 2 hash rounds per 4 elements where uniform01() needs 12 (the hash was most of the VALU work of the LayerNorm kernels: 14 + 14 launches a step).
// keep iff u16 >= p * 65536.  Every kernel that must agree on a mask calls these two functions with the same (seed, salt, quad index).
// The salt (one per dropout site) enters the FIRST round: every word of the draw -- hence every element of the quad -- differs between two sites
// that share the step's seed and the flat index (round 5 kept it out of h[0]: elements 0 and 1 of every quad had the same mask at every site).
EMRT_DROP_FN void drop_quad(uint64_t seed, uint32_t salt, uint64_t quad, uint32_t (&h)[2]) {
  h[0] = mix32(((uint32_t)quad ^ (uint32_t)seed) + salt * 0x9E3779B9U);
  h[1] = mix32(h[0] ^ (uint32_t)(quad >> 32) ^ (uint32_t)(seed >> 32) ^ (salt * 0x85EBCA6BU));
}
EMRT_DROP_FN bool drop_quad_keep(const uint32_t (&h)[2], int e, uint32_t thr) { return ((h[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= thr; }
EMRT_DROP_FN uint32_t drop_thr16(float p) { return (uint32_t)(p * 65536.f); }

// Dropout inside a GEMM epilogue (conv.hip: linear1 -> ReLU -> Dropout of the FFN): the per-element hash above costs ~45 VALU instructions
// per element, which on a GEMM's critical path cost more than the separate dropout launch it replaced.  Here ONE group of
// 8 consecutive channels of a row draws four 32-bit words = eight 16-bit uniforms (~4 instructions per element); keep iff u16 >= p * 65536.
// The backward never re-derives this mask: the consumer's data gradient masks with (stored output > 0) (functional.conv2d: drop_rec).
EMRT_DROP_FN void drop_words8(uint64_t seed, uint32_t salt, uint32_t group, uint32_t (&h)[4]) {
  h[0] = mix32((group ^ (uint32_t)seed) + salt * 0x9E3779B9U);      // (the salt in the first round: see drop_quad)
  h[1] = mix32(h[0] ^ (uint32_t)(seed >> 32) ^ (salt * 0x85EBCA6BU));
  h[2] = mix32(h[1] + 0x9E3779B9U + (h[0] << 6));
  h[3] = mix32(h[2] ^ 0x85EBCA6BU ^ (h[1] >> 2));
}
EMRT_DROP_FN bool drop_keep8(const uint32_t (&h)[4], int e, uint32_t thr) { return ((h[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= thr; }

// Attention (attn.hip, the MFMA kernels): four 16-bit uniforms for (row, quad of 4 consecutive columns); keep iff u16 >= thr
EMRT_DROP_FN void mha_drop4(unsigned long long seed, unsigned salt, unsigned group, uint32_t (&h)[2]) {
  h[0] = mix32((group ^ (uint32_t)seed) + salt * 0x9E3779B9U);      // (the salt in the first round: see drop_quad)
  h[1] = mix32(h[0] ^ (uint32_t)(seed >> 32) ^ (salt * 0x85EBCA6BU));
}
EMRT_DROP_FN bool mha_keep4(const uint32_t (&h)[2], int e, uint32_t thr) { return ((h[e >> 1] >> (16 * (e & 1))) & 0xffffu) >= thr; }

}  // namespace emrt
