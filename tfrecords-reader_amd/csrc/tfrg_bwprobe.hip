// tfrg_bwprobe.hip — k_stream_read: a streaming read of a device buffer, the achievable HBM read
// bandwidth that bench.py reports beside the decode (measurement only; no part of a decode).
#include "tfrg_internal.h"

namespace tfrg {

// Streaming read (measurement only): each block reads a contiguous slab, U 16-byte loads in flight
// per lane (all issued before any is consumed), nontemporal (the data is not reused).
typedef uint32_t sr_u32x4 __attribute__((ext_vector_type(4)));
template <int U>
__global__ __launch_bounds__(256) void k_stream_read(const sr_u32x4* __restrict__ p, uint64_t n16, uint32_t* sink) {
  uint32_t acc = 0;
  const uint64_t per_block = (n16 + gridDim.x - 1) / gridDim.x;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
  const uint64_t b1 = b0 + per_block < n16 ? b0 + per_block : n16;
  uint64_t i = b0 + threadIdx.x;
  for (; i + (U - 1) * 256 < b1; i += U * 256) {
    sr_u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(p + i + u * 256);
#pragma unroll
    for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
  }
  for (; i < b1; i += 256) {
    const sr_u32x4 a = p[i];
    acc ^= a.x ^ a.y ^ a.z ^ a.w;
  }
  if (acc == 0x9e3779b9u) atomicXor(sink, acc);  // practically never taken; keeps the loads live
}

// variant: 0 = 4 loads in flight, 16 blocks per CU; 1 = 8 loads, 8 blocks per CU; 2 = 8 loads, 16
// blocks per CU; 3 = 16 loads, 4 blocks per CU (bench.py reports the fastest)
hipError_t launch_stream_read(const void* d, uint64_t nbytes, uint32_t* sink, hipStream_t st, int variant) {
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const sr_u32x4* q = static_cast<const sr_u32x4*>(d);
  switch (variant) {
    case 0: hipLaunchKernelGGL(k_stream_read<4>, dim3(cus * 16), dim3(256), 0, st, q, nbytes / 16, sink); break;
    case 1: hipLaunchKernelGGL(k_stream_read<8>, dim3(cus * 8), dim3(256), 0, st, q, nbytes / 16, sink); break;
    case 2: hipLaunchKernelGGL(k_stream_read<8>, dim3(cus * 16), dim3(256), 0, st, q, nbytes / 16, sink); break;
    default: hipLaunchKernelGGL(k_stream_read<16>, dim3(cus * 4), dim3(256), 0, st, q, nbytes / 16, sink); break;
  }
  return hipGetLastError();
}

}  // namespace tfrg
