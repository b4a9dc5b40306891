// transforms.Normalize's arithmetic on a uint8 sample, written once: scene.hip (emrt_scene_crop_windows_u8) and tta_ext/tta_ext.hip
// (emrt_tta_crop_windows_u8) compile this text, so both make the bits the CPU transform makes.
#pragma once
#include <hip/hip_runtime.h>

namespace emrt {

struct SceneNorm {
  double mean[3], stdinv[3];
};

// float64 math, one rounding
__device__ __forceinline__ float normalise_u8(unsigned v, double mean, double stdinv) { return (float)(((double)v - mean) * stdinv); }

// the same arithmetic on a sample that has been resampled in fp32 (mstta_ext/mstta_ext.hip): on a whole number, normalise_u8's bits
__device__ __forceinline__ float normalise_f32(float v, double mean, double stdinv) { return (float)(((double)v - mean) * stdinv); }

}  // namespace emrt
