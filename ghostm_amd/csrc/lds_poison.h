// lds_poison.h — the LDS poison build's prologue (device.hip and index.hip).
//
// LDS poison build (-DGHOSTM_LDS_POISON=1, ghostm_amd/lib/libghostm_hip_poison.so):
// every kernel first fills its whole LDS allocation, static and dynamic (the
// dispatch packet's group_segment_size), with g_lds_poison, so a read of LDS
// the kernel never wrote returns that pattern instead of whatever an earlier
// workgroup left there. Tests run the golden variants under two patterns: a
// result that depends on such a read differs under one of them.
// g_lds_poison is one variable per translation unit; each sets its own from
// GHOSTM_LDS_POISON_PATTERN before its first launch (LdsPoisonPattern).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

namespace ghostm {
namespace kern {

#ifdef GHOSTM_LDS_POISON
static __device__ uint32_t g_lds_poison = 0xA5A5A5A5u;
__device__ __forceinline__ void PoisonLds() {
  // hsa_kernel_dispatch_packet_t: group_segment_size at byte 28
  typedef const __attribute__((address_space(4))) uint32_t *PacketWords;
  const uint32_t bytes = ((PacketWords)__builtin_amdgcn_dispatch_ptr())[7];
  const uint32_t v = g_lds_poison;
  const uint32_t nthreads = blockDim.x * blockDim.y * blockDim.z;
  const uint32_t tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
  for (uint32_t off = tid * 4; off + 4 <= bytes; off += nthreads * 4)
    asm volatile("ds_write_b32 %0, %1" : : "v"(off), "v"(v) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");
  __syncthreads();
}
// the pattern every kernel writes over its LDS before its own code runs
inline uint32_t LdsPoisonPattern() {
  const char *e = getenv("GHOSTM_LDS_POISON_PATTERN");
  return e ? (uint32_t)strtoul(e, nullptr, 0) : 0xA5A5A5A5u;
}
#define GHOSTM_POISON_LDS() ::ghostm::kern::PoisonLds()
#else
#define GHOSTM_POISON_LDS() ((void)0)
#endif

}  // namespace kern
}  // namespace ghostm
