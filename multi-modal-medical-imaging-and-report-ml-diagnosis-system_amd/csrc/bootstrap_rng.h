// The bootstrap resampling stream: counter-based and stateless.  Draw k of replicate r of an
// N-row resample is the row index
//     boot_draw(boot_key(seed, r), k, N)
// and depends on (seed, r, k, N) alone: not on how many replicates a launch makes, on batching
// or on the launch shape.  mmdx/bootstrap.py (reference_weights) restates it in numpy; the two
// must stay equal bit for bit.  This is NOT the dropout stream (dropout_rng.h): another hash,
// another key schedule, and nothing here advances a device counter.
//
//   mix64  = the SplitMix64 output function (shifts 30 / 27 / 31)
//   key_r  = mix64(seed ^ ((r + 1) * GOLDEN))
//   h      = mix64(key_r + (k + 1) * GOLDEN)
//   idx    = mulhi64(h, N)        range reduction with bias N / 2^64
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmdx {

constexpr uint64_t BOOT_GOLDEN = 0x9E3779B97F4A7C15ULL;

__host__ __device__ inline uint64_t boot_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t boot_key(uint64_t seed, uint64_t r) {
  return boot_mix64(seed ^ ((r + 1) * BOOT_GOLDEN));
}
__host__ __device__ inline uint64_t boot_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// row index in [0, N)
__host__ __device__ inline uint32_t boot_draw(uint64_t key, uint64_t k, uint32_t N) {
  return (uint32_t)boot_mulhi64(boot_mix64(key + (k + 1) * BOOT_GOLDEN), N);
}

}  // namespace mmdx
