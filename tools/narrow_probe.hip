// Tuning aid: what can the LOADS of the narrow dense scan reach by themselves? Streams the headline's columns — a 1-byte index column, a
// 2-byte index column, a float64 column, two validity bitmaps: 11.25 B per row — with nothing behind the loads but an xor, in five forms:
//   wide4   the 4-byte scan's pattern (two uint32 index columns: 16.25 B per row), a lane owns 4 rows: 16 B + 16 B + 2 × 16 B per lane
//   direct  the narrow scan's pattern (fdb_jitgen.cpp, ld1x4 / ld2x4), a lane owns 4 rows: 4 B + 8 B + 2 × 16 B per lane
//   wide16  a lane owns 16 consecutive rows: 16 B + 2 × 16 B + 8 × 16 B per lane (every index load a full 16-byte load)
//   quad16  a wave owns a block of 1 024 rows as four sub-steps of 256 rows, in sub-step u lane l owns rows 256u + 4l … +3, and the index columns
//           are read as if laid out for that (a wave-interleaved cache): one 16-byte load at 16l of the block's 1 024 B of the 1-byte column,
//           two at 1024h + 16l of its 2 048 B of the 2-byte column, eight value loads at 32l and 32l + 16 of each sub-step's 2 KiB, and the
//           validity bytes as `direct` loads them; all of a block's loads leave before the xor
//   quad16m quad16 with each bitmap's 128 B of the block read as one dword per lane and a cross-lane read per sub-step
// Persistent grid, tiles taken grid-stride, non-temporal loads, `waves` workgroups of 256 threads per CU.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/narrow_probe.hip -o tools/narrow_probe && tools/narrow_probe [rows] [workgroups per CU ...]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define G1 __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ T ldnt(const void* base, size_t byte_off) {
  return __builtin_nontemporal_load((const G1 T*)(reinterpret_cast<const char*>(base) + byte_off));
}

struct Cols { const void* c1; const void* c2; const void* v; const uint8_t* b1; const uint8_t* b2; long long rows; unsigned long long* sink; };

// MODE 0: wide4 (c1 and c2 hold uint32), 1: direct, 2: wide16, 3: quad16, 4: quad16m
template <int MODE>
__global__ __launch_bounds__(256) void probe_kernel(Cols c) {
  constexpr int RPL = MODE >= 2 ? 16 : 4;  // rows per lane and tile
  const long long tile_rows = 256LL * RPL, tiles = c.rows / tile_rows;  // (rows is a multiple of 4 096: no tail)
  const uint32_t tid = threadIdx.x;
  uint32_t acc = 0;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t row = (size_t)tile * tile_rows + (size_t)tid * RPL;
    if (MODE == 0) {
      const u32x4 a = ldnt<u32x4>(c.c1, row * 4), b = ldnt<u32x4>(c.c2, row * 4);
      const u32x4 v0 = ldnt<u32x4>(c.v, row * 8), v1 = ldnt<u32x4>(c.v, row * 8 + 16);
      const uint32_t m1 = ((const G1 uint8_t*)c.b1)[row >> 3], m2 = ((const G1 uint8_t*)c.b2)[row >> 3];
      acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ v0.x ^ v0.y ^ v0.z ^ v0.w ^ v1.x ^ v1.y ^ v1.z ^ v1.w ^ m1 ^ m2;
    } else if (MODE == 1) {
      const uint32_t a = ldnt<uint32_t>(c.c1, row);
      const u32x2 b = ldnt<u32x2>(c.c2, row * 2);
      const u32x4 v0 = ldnt<u32x4>(c.v, row * 8), v1 = ldnt<u32x4>(c.v, row * 8 + 16);
      const uint32_t m1 = ((const G1 uint8_t*)c.b1)[row >> 3], m2 = ((const G1 uint8_t*)c.b2)[row >> 3];
      acc ^= a ^ b.x ^ b.y ^ v0.x ^ v0.y ^ v0.z ^ v0.w ^ v1.x ^ v1.y ^ v1.z ^ v1.w ^ m1 ^ m2;
    } else if (MODE >= 3) {
      const uint32_t lane = tid & 63u;
      const size_t blk = (size_t)tile * tile_rows + (size_t)(tid >> 6) * 1024;  // the wave's block of 1 024 rows
      const u32x4 a = ldnt<u32x4>(c.c1, blk + 16 * lane);
      const u32x4 b0 = ldnt<u32x4>(c.c2, blk * 2 + 16 * lane), b1 = ldnt<u32x4>(c.c2, blk * 2 + 1024 + 16 * lane);
      u32x4 v[8];
      uint32_t m = 0;
      if (MODE == 4) m = ((const G1 uint32_t*)c.b1)[(blk >> 5) + (lane & 31u)] ^ (((const G1 uint32_t*)c.b2)[(blk >> 5) + (lane & 31u)] << 1);
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const size_t r = blk + 256 * u + 4 * lane;
        v[2 * u] = ldnt<u32x4>(c.v, r * 8);
        v[2 * u + 1] = ldnt<u32x4>(c.v, r * 8 + 16);
        if (MODE == 3) m ^= ((const G1 uint8_t*)c.b1)[r >> 3] ^ ((uint32_t)((const G1 uint8_t*)c.b2)[r >> 3] << (8 * u));
      }
      if (MODE == 4) {
        uint32_t x = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) x ^= (uint32_t)__shfl((int)m, 8 * u + (int)(lane >> 3)) >> (4 * (lane & 7u));  // sub-step u's bits of rows 4l … 4l+3
        m = x;
      }
      acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b0.x ^ b0.y ^ b0.z ^ b0.w ^ b1.x ^ b1.y ^ b1.z ^ b1.w ^ m;
#pragma unroll
      for (int k = 0; k < 8; k++) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    } else {
      const u32x4 a = ldnt<u32x4>(c.c1, row);
      const u32x4 b0 = ldnt<u32x4>(c.c2, row * 2), b1 = ldnt<u32x4>(c.c2, row * 2 + 16);
      u32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = ldnt<u32x4>(c.v, row * 8 + 16 * k);
      const uint32_t m1 = ((const G1 uint16_t*)c.b1)[row >> 4], m2 = ((const G1 uint16_t*)c.b2)[row >> 4];
      acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b0.x ^ b0.y ^ b0.z ^ b0.w ^ b1.x ^ b1.y ^ b1.z ^ b1.w ^ m1 ^ m2;
#pragma unroll
      for (int k = 0; k < 8; k++) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    }
  }
  if (acc == 0x9E3779B9u) c.sink[0] = 1;  // keeps the loads alive; never true for the zero-filled buffers
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  long long rows = argc > 1 ? std::atoll(argv[1]) : 400000000LL;
  rows = rows / 4096 * 4096;
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const size_t pad = 4096;
  void *c1, *c2, *v; uint8_t *b1, *b2; unsigned long long* sink;
  CK(hipMalloc(&c1, (size_t)rows * 4 + pad)); CK(hipMalloc(&c2, (size_t)rows * 4 + pad)); CK(hipMalloc(&v, (size_t)rows * 8 + pad));
  CK(hipMalloc((void**)&b1, (size_t)rows / 8 + pad)); CK(hipMalloc((void**)&b2, (size_t)rows / 8 + pad)); CK(hipMalloc((void**)&sink, 8));
  CK(hipMemset(c1, 0, (size_t)rows * 4 + pad)); CK(hipMemset(c2, 0, (size_t)rows * 4 + pad)); CK(hipMemset(v, 0, (size_t)rows * 8 + pad));
  CK(hipMemset(b1, 0, (size_t)rows / 8 + pad)); CK(hipMemset(b2, 0, (size_t)rows / 8 + pad)); CK(hipMemset(sink, 0, 8));
  Cols c{c1, c2, v, b1, b2, rows, sink};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char* names[5] = {"wide4  ", "direct ", "wide16 ", "quad16 ", "quad16m"};
  const double bytes_per_row[5] = {16.25, 11.25, 11.25, 11.25, 11.25};
  const int per_cu_list[4] = {4, 6, 8, 2};
  for (int pi = 0; pi < (argc > 2 ? argc - 2 : 4); pi++) {
    const int per_cu = argc > 2 ? std::atoi(argv[2 + pi]) : per_cu_list[pi];
    if (per_cu < 1 || per_cu > 8) { std::fprintf(stderr, "workgroups per CU: 1 to 8\n"); return 1; }
    for (int mode = 0; mode < 5; mode++) {
      float best = 1e30f;
      for (int rep = 0; rep < 7; rep++) {
        CK(hipEventRecord(e0, 0));
        if (mode == 0) hipLaunchKernelGGL(probe_kernel<0>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 1) hipLaunchKernelGGL(probe_kernel<1>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 2) hipLaunchKernelGGL(probe_kernel<2>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 3) hipLaunchKernelGGL(probe_kernel<3>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else hipLaunchKernelGGL(probe_kernel<4>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= 2 && ms < best) best = ms;
      }
      std::printf("%s  %d workgroups/CU  %lld rows  %.4f ms  %.0f GB/s  (%.2f B/row)\n", names[mode], per_cu, rows, best, bytes_per_row[mode] * rows / (best * 1e-3) / 1e9, bytes_per_row[mode]);
    }
  }
  return 0;
}
