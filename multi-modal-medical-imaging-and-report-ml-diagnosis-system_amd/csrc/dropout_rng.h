// The library's one dropout stream: a counter-based hash, no state on the device but a launch
// counter.  Element `idx` of the tensor a kernel drops is kept when
//     dropout_keep(dropout_stream_base(seed, counter), idx, p)
// and each consuming launch is followed, on the same stream, by one dropout_counter_advance(),
// so the next launch (or the next replay of a captured graph) draws fresh bits.
//
// Contract: kernels that must agree on a mask draw it through these functions from the same
// (seed, counter value, element index), and nothing else enters the draw:
//  * attn_fwd_kernel / attn_fwd16_kernel (P-saving and flash-style forwards) draw the same mask
//    for the same call, so switching MMDX_ATTN_FLASH does not change a training run;
//  * attn_bwd_q16_lse_kernel and attn_bwd_kv16_lse_kernel redraw the forward's keep bits instead
//    of reading a saved mask: the forward leaves its stream base in rng[0], and both index
//    element ((b*H + h)*L + q)*L + key;
//  * ln_fwd_kernel<DROP> / ln_bwd_kernel<DROP> promise rows bit-identical to mmdx_dropout_fwd
//    followed by mmdx_layernorm_fwd: both index the flat element row*D + c;
//  * xattn_fwd_kernel indexes ((b*H + h)*Lq + q)*Lk + key.
// The element-index formulas stay at the call sites; the stream is defined here alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmdx {

// 64 -> 32 bit mix (the murmur3 finaliser)
__device__ __forceinline__ uint32_t dropout_mix(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (uint32_t)x;
}
// base of the launch's stream: the seed spread by the 64-bit golden ratio, the device launch
// counter in the high half (a null counter: the seed alone)
__device__ __forceinline__ uint64_t dropout_stream_base(uint64_t seed, const uint64_t* ctr) {
  return seed * 0x9E3779B97F4A7C15ULL + (ctr ? ctr[0] << 32 : 0ull);
}
// uniform in [0, 1) with 24 bits, exact in fp32
__device__ __forceinline__ float dropout_uniform(uint64_t base, uint64_t idx) {
  return (dropout_mix(base + idx) >> 8) * (1.f / 16777216.f);
}
__device__ __forceinline__ bool dropout_keep(uint64_t base, uint64_t idx, float p) {
  return dropout_uniform(base, idx) >= p;
}

// counter[0] += 1 as a one-thread launch on `stream` (the kernel lives in misc.hip)
void dropout_counter_advance(uint64_t* counter, hipStream_t stream);

}  // namespace mmdx
