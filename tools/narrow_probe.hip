// Tuning aid: what can the LOADS of the narrow dense scan reach by themselves? Streams the headline's columns — a 1-byte index column, a
// 2-byte index column, a float64 column, two validity bitmaps: 11.25 B per row — with nothing behind the loads but an xor, in five forms (three more, behind the null-folded cache, at packed_kernel below):
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

// The forms behind the null-folded cache (no bitmap is loaded any more), each unpacking all 16 rows' two indices and keeping them alive with one
// LDS gather each, as the generated kernel's LUT lookups do. Index buffers hold pseudo-random indices below 8 and below 1 024 in every form.
//   FORM 0  quad16f  what the dense scan reads today: quad16 without the bitmaps, 1 + 2 + 8 loads of 16 bytes: 11 B per row
//   FORM 1  pack16   `code` at 4 bits (a frame of 512 B per block: the lane's 16 nibbles are the 8 bytes at 8l, sub-step u bits 16u … 16u + 15) and
//                    `path` at 12 bits (a frame of 1 536 B: the low bytes laid out as the 1-byte column, then 512 B of high nibbles laid out
//                    as `code`): 8 + 16 + 8 bytes of indices and 8 value loads, 10 B per row
//   FORM 2  pack16w  pack16 with no 8-byte load: a wave owns two consecutive blocks, whose nibble planes sit side by side (block 0's word in
//                    dwords 0 – 1 of the lane's 16 bytes, block 1's in dwords 2 – 3); 1 + 3 + 16 loads of 16 bytes per 2 048 rows
struct Packed { const void* q1; const void* q2; const void* p1; const void* p2; const void* v; long long rows; unsigned long long* sink; };

template <int FORM>
__global__ __launch_bounds__(256) void packed_kernel(Packed c) {
  constexpr int BLOCKS = FORM == 2 ? 2 : 1;  // blocks of 1 024 rows per wave and tile
  __shared__ uint32_t lut1[16], lut2[1024];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t i = tid; i < 1024; i += 256) lut2[i] = i * 0x9E3779B1u;
  if (tid < 16) lut1[tid] = tid * 0x85EBCA77u;
  __syncthreads();
  const long long tile_rows = 4096LL * BLOCKS, tiles = c.rows / tile_rows;
  uint32_t acc = 0;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t blk = (size_t)tile * tile_rows + (size_t)(tid >> 6) * 1024 * BLOCKS;  // the wave's first row
    u32x4 a[BLOCKS], v[8 * BLOCKS];
    u32x4 b0, b1;   // quad16f: the 2-byte column's two halves
    u32x2 n1, n2;   // pack16: the lane's nibbles of `code` and of `path`
    u32x4 w1, w2;   // pack16w: the same for two blocks
    if (FORM == 0) {
      a[0] = ldnt<u32x4>(c.q1, blk + 16 * lane);
      b0 = ldnt<u32x4>(c.q2, blk * 2 + 16 * lane), b1 = ldnt<u32x4>(c.q2, blk * 2 + 1024 + 16 * lane);
    } else if (FORM == 1) {
      n1 = ldnt<u32x2>(c.p1, blk / 2 + 8 * lane);
      a[0] = ldnt<u32x4>(c.p2, blk / 1024 * 1536 + 16 * lane);
      n2 = ldnt<u32x2>(c.p2, blk / 1024 * 1536 + 1024 + 8 * lane);
    } else {
      w1 = ldnt<u32x4>(c.p1, blk / 2 + 16 * lane);
#pragma unroll
      for (int k = 0; k < BLOCKS; k++) a[k] = ldnt<u32x4>(c.p2, blk / 2048 * 3072 + 1024 * k + 16 * lane);
      w2 = ldnt<u32x4>(c.p2, blk / 2048 * 3072 + 2048 + 16 * lane);
    }
#pragma unroll
    for (int u = 0; u < 4 * BLOCKS; u++) {
      const size_t r = blk + 256 * u + 4 * lane;
      v[2 * u] = ldnt<u32x4>(c.v, r * 8);
      v[2 * u + 1] = ldnt<u32x4>(c.v, r * 8 + 16);
    }
    asm volatile("" :: "v"(v[0]), "v"(v[1]));  // as Gen::block_loads ends: the scheduler leaves every load in front of the first use
#pragma unroll
    for (int u = 0; u < 4 * BLOCKS; u++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        uint32_t i1, i2;
        if (FORM == 0) {
          i1 = (a[0][u] >> (8 * r)) & 0xFFu;
          i2 = ((u < 2 ? b0 : b1)[2 * (u & 1) + r / 2] >> (16 * (r & 1))) & 0xFFFFu;
        } else {
          const uint32_t h1 = FORM == 1 ? n1[u >> 1] : w1[u >> 1], h2 = FORM == 1 ? n2[u >> 1] : w2[u >> 1];
          const int bit = 16 * (u & 1) + 4 * r;
          i1 = (h1 >> bit) & 0xFu;
          i2 = ((a[u >> 2][u & 3] >> (8 * r)) & 0xFFu) | (((h2 >> bit) & 0xFu) << 8);
        }
        acc ^= lut1[i1] ^ lut2[i2];
      }
      acc ^= v[2 * u].x ^ v[2 * u].y ^ v[2 * u].z ^ v[2 * u].w ^ v[2 * u + 1].x ^ v[2 * u + 1].y ^ v[2 * u + 1].z ^ v[2 * u + 1].w;
    }
  }
  if (acc == 0x9E3779B9u) c.sink[0] = 1;  // keeps the loads and the gathers alive; the value column is zero-filled, the LUT words are not
}

// Pseudo-random bytes under a per-byte mask: every index the packed forms unpack stays inside its LUT.
// A buffer of frames (`frame` words, the first `plane` of them a byte plane under `mask`, the rest a nibble plane under `mask2`).
__global__ void fill_kernel(uint32_t* p, size_t words, uint32_t mask, uint32_t frame, uint32_t plane, uint32_t mask2) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t x = (uint32_t)i * 0x9E3779B1u + (uint32_t)(i >> 32);
    x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 12;
    p[i] = x & (i % frame < plane ? mask : mask2);
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  long long rows = argc > 1 ? std::atoll(argv[1]) : 400000000LL;
  rows = rows / 8192 * 8192;  // whole tiles of every form
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
  void *q1, *q2, *p1, *p2;  // the folded forms' index buffers: 1 and 2 bytes per index, 4 bits and 12 bits per index
  CK(hipMalloc(&q1, (size_t)rows + pad)); CK(hipMalloc(&q2, (size_t)rows * 2 + pad));
  CK(hipMalloc(&p1, (size_t)rows / 2 + pad)); CK(hipMalloc(&p2, (size_t)rows / 2 * 3 + pad));
  hipLaunchKernelGGL(fill_kernel, dim3(cus * 8), dim3(256), 0, 0, (uint32_t*)q1, (size_t)rows / 4, 0x07070707u, 1u, 1u, 0u);
  hipLaunchKernelGGL(fill_kernel, dim3(cus * 8), dim3(256), 0, 0, (uint32_t*)q2, (size_t)rows / 2, 0x03FF03FFu, 1u, 1u, 0u);
  hipLaunchKernelGGL(fill_kernel, dim3(cus * 8), dim3(256), 0, 0, (uint32_t*)p1, (size_t)rows / 8, 0x77777777u, 1u, 1u, 0u);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  Packed pc{q1, q2, p1, p2, v, rows, sink};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char* names[8] = {"wide4  ", "direct ", "wide16 ", "quad16 ", "quad16m", "quad16f", "pack16 ", "pack16w"};
  const double bytes_per_row[8] = {16.25, 11.25, 11.25, 11.25, 11.25, 11.0, 10.0, 10.0};
  const int per_cu_list[4] = {4, 6, 8, 2};
  for (int pi = 0; pi < (argc > 2 ? argc - 2 : 4); pi++) {
    const int per_cu = argc > 2 ? std::atoi(argv[2 + pi]) : per_cu_list[pi];
    if (per_cu < 1 || per_cu > 8) { std::fprintf(stderr, "workgroups per CU: 1 to 8\n"); return 1; }
    for (int mode = 0; mode < 8; mode++) {
      if (mode >= 6) {  // the 12-bit buffer's frames: one block's (1 024 B + 512 B) or two blocks' (2 048 B + 1 024 B)
        const uint32_t k = mode == 6 ? 1u : 2u;
        hipLaunchKernelGGL(fill_kernel, dim3(cus * 8), dim3(256), 0, 0, (uint32_t*)p2, (size_t)rows / 8 * 3, 0xFFFFFFFFu, 384u * k, 256u * k, 0x33333333u);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
      }
      float best = 1e30f;
      for (int rep = 0; rep < 7; rep++) {
        CK(hipEventRecord(e0, 0));
        if (mode == 0) hipLaunchKernelGGL(probe_kernel<0>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 1) hipLaunchKernelGGL(probe_kernel<1>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 2) hipLaunchKernelGGL(probe_kernel<2>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 3) hipLaunchKernelGGL(probe_kernel<3>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 4) hipLaunchKernelGGL(probe_kernel<4>, dim3(cus * per_cu), dim3(256), 0, 0, c);
        else if (mode == 5) hipLaunchKernelGGL(packed_kernel<0>, dim3(cus * per_cu), dim3(256), 0, 0, pc);
        else if (mode == 6) hipLaunchKernelGGL(packed_kernel<1>, dim3(cus * per_cu), dim3(256), 0, 0, pc);
        else hipLaunchKernelGGL(packed_kernel<2>, dim3(cus * per_cu), dim3(256), 0, 0, pc);
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
