// Philox4x32-10 and the draws made from its words, shared by every kernel that takes a random decision on the device: emrt_scene_draw
// (augment.hip), emrt_aug_scene_draw (augment_ext/augment_ext.hip), emrt_smp_class_redraw (sampler_ext/sampler_ext.hip) and emrt_rot_scene_batch
// (rot_ext/rot_ext.hip).  One text, so the libraries cannot drift apart: a sample's blocks are numbered across all of them (include/emrt_hip_rot.h
// lists who owns which).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants):
//   key = (key64 low word, key64 high word);  counter = (step low word, step high word, rank * B + b, j),  j = the sample's j-th 128-bit block
// A 64-bit value is two output words, (w[2k + 1] << 32) | w[2k]; a uniform integer below n is the high half of value * n (bias < n * 2^-64).
#pragma once
#include <hip/hip_runtime.h>

namespace emrt {

struct Philox {
  unsigned v[4];
};

__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

__device__ __forceinline__ unsigned long long below(unsigned lo, unsigned hi, unsigned long long n) {
  return __umul64hi(((unsigned long long)hi << 32) | lo, n);
}

// a word as a float64 in [0, 1): exact, 32 bits
__device__ __forceinline__ double unit(unsigned w) { return (double)w * (1.0 / 4294967296.0); }

}  // namespace emrt
