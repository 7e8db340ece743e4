// frostdb_amd — compressed Parquet pages → bytes on the device (see fdb_kernels.h): snappy_decode_kernel and lz4_decode_kernel, one wave
// per page, over one page-stream core (PageStream): the LDS input window, the LDS output ring with its segment flush, the literal copy
// and the match copy. A kernel holds its format's grammar and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fdb_kernels.h"

namespace {
constexpr uint32_t PAGE_WIN = 2048;    // bytes of the compressed stream held in LDS
constexpr uint32_t PAGE_RING = 65536;  // the page's most recent output, in LDS: what copies read (a compressor's matches stay inside its 64 KiB fragment)
constexpr uint32_t PAGE_SEG = 16384;   // the ring goes to HBM a segment at a time, 16 bytes per lane
constexpr uint32_t PAGE_LDS = PAGE_WIN + 16 + PAGE_RING;
static_assert(FDB_PAGE_RING_REACH == PAGE_RING - 64u, "the host's gate and the kernels agree on how far back a copy may reach");
struct __attribute__((packed, aligned(1))) Chunk16 { unsigned long long a, b; };  // 16 bytes at any address
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One page as a stream: compressed bytes in through the window, output through the ring. n, cap, base, ip, op, flushed and err are
// wave-uniform; every member is inlined into the kernel, where the state lives in (mostly scalar) registers.
// First version: copies read the page's output back from HBM — correct, and 0.56 µs per ELEMENT (a dependent global round trip each):
// 11 MB/s per page of dictionary indices. Elements now touch LDS only: tags come out of the input window, copies read and write the
// output ring, and the ring leaves for HBM in 16 KiB segments.
struct PageStream {
  uint8_t* const win;   // [PAGE_WIN + 16]
  uint8_t* const ring;  // [PAGE_RING]
  const uint8_t* const in;
  uint8_t* const out;
  const uint32_t n, cap, lane;
  uint32_t base = 0xFFFFFFFFu, ip = 0, op = 0, flushed = 0, err = 0;

  __device__ __forceinline__ PageStream(unsigned char* smem, const uint8_t* src, uint8_t* dst, const FdbCodecPage& P)
      : win(smem), ring(smem + PAGE_WIN + 16), in(src + P.src_off), out(dst + P.dst_off), n((uint32_t)__builtin_amdgcn_readfirstlane((int)P.src_len)),
        cap((uint32_t)__builtin_amdgcn_readfirstlane((int)P.dst_len)), lane(threadIdx.x) {}

  // the window = bytes [at, at + PAGE_WIN) of the stream (zeros past its end: the bounds are checked on ip, not here)
  __device__ __forceinline__ void refill(const uint32_t at) {
    __builtin_amdgcn_wave_barrier();
    base = at;
    const uint32_t i = lane * 32u;  // 64 lanes × 32 bytes
    Chunk16 c0 = {0ull, 0ull}, c1 = {0ull, 0ull};
    if ((unsigned long long)base + i + 32u <= n) { c0 = *reinterpret_cast<const Chunk16*>(in + base + i); c1 = *reinterpret_cast<const Chunk16*>(in + base + i + 16); }
    else {
      uint8_t t[32];
      for (uint32_t k = 0; k < 32u; k++) t[k] = (unsigned long long)base + i + k < n ? in[base + i + k] : (uint8_t)0;
      __builtin_memcpy(&c0, t, 16); __builtin_memcpy(&c1, t + 16, 16);
    }
    *reinterpret_cast<Chunk16*>(win + i) = c0; *reinterpret_cast<Chunk16*>(win + i + 16) = c1;
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ bool in_window(const uint32_t at, const uint32_t need) const { return base != 0xFFFFFFFFu && at >= base && at - base <= PAGE_WIN - need; }
  // bytes [at, at + 8) of the stream, wave-uniform (three aligned words; the window has a word of slack behind it)
  __device__ __forceinline__ unsigned long long fetch(const uint32_t at) {
    if (!in_window(at, 8u)) refill(at);
    const uint32_t o = at - base, sh = (o & 3u) * 8u;
    const uint32_t* w32 = reinterpret_cast<const uint32_t*>(win + (o & ~3u));
    const uint32_t w0 = w32[0], w1 = w32[1], w2 = w32[2];
    unsigned long long v = ((unsigned long long)w1 << 32) | w0;
    if (sh != 0u) v = (v >> sh) | ((unsigned long long)w2 << (64u - sh));
    // every lane read the same bytes: say so, and the tag arithmetic and the branches on it run on the scalar unit
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
  }
  // ring → HBM: every segment that is complete (all == false), or everything up to op (the page's end)
  __device__ __forceinline__ void flush(const bool all) {
    __builtin_amdgcn_wave_barrier();
    while (flushed + PAGE_SEG <= op) {
      const uint32_t r0 = flushed & (PAGE_RING - 1u);
      for (uint32_t i = lane * 16u; i < PAGE_SEG; i += 64u * 16u) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ring + r0 + i);
        Chunk16 c; __builtin_memcpy(&c, &v, 16);
        *reinterpret_cast<Chunk16*>(out + flushed + i) = c;
      }
      flushed += PAGE_SEG;
    }
    if (all) { for (uint32_t i = flushed + lane; i < op; i += 64u) out[i] = ring[i & (PAGE_RING - 1u)]; flushed = op; }
    __builtin_amdgcn_wave_barrier();
  }
  // l literal bytes at stream position `from` → the ring; ip ends behind them. The caller has checked from + l ≤ n and op + l ≤ cap.
  __device__ __forceinline__ void literals(const uint32_t from, const uint32_t l) {
    if (l <= PAGE_WIN && in_window(from, l)) {  // short and already in the window
      for (uint32_t i = lane; i < l; i += 64u) ring[(op + i) & (PAGE_RING - 1u)] = win[from - base + i];
      op += l;
    } else {  // from the stream in HBM, at most what the ring has room for at a time (it must not lap what has not been flushed)
      uint32_t done = 0;
      while (done < l) {
        const uint32_t room = PAGE_RING - (op - flushed), take = l - done < room ? l - done : room;
        const uint32_t body = take & ~15u;
        for (uint32_t i = lane * 16u; i < body; i += 64u * 16u) {
          const Chunk16 c = *reinterpret_cast<const Chunk16*>(in + from + done + i);
          uint8_t t[16]; __builtin_memcpy(t, &c, 16);
          const uint32_t r = (op + i) & (PAGE_RING - 1u);
          if ((r & 15u) == 0u) { u32x4 v; __builtin_memcpy(&v, t, 16); *reinterpret_cast<u32x4*>(ring + r) = v; }
          else { for (uint32_t k = 0; k < 16u; k++) ring[(r + k) & (PAGE_RING - 1u)] = t[k]; }
        }
        for (uint32_t i = body + lane; i < take; i += 64u) ring[(op + i) & (PAGE_RING - 1u)] = in[from + done + i];
        op += take; done += take;
        if (op - flushed >= PAGE_SEG) flush(false);
      }
    }
    ip = from + l;
    if (op - flushed >= 2u * PAGE_SEG) flush(false);
  }
  // len bytes from `off` bytes back (0 < off ≤ min(op, FDB_PAGE_RING_REACH), op + len ≤ cap: the caller's checks) → the ring, 64 bytes
  // at a time, one per lane: everything up to the chunk's first byte is in the ring, so byte i of the chunk is the byte `off` before it —
  // or, where the pattern is shorter than the chunk, byte (i mod off) of the `off` bytes before the chunk. off and len are wave-uniform:
  // the cases are BRANCHES (as one select the division of the rare case was paid by every element), and the division is done once per match
  __device__ __forceinline__ void match(const uint32_t off, const uint32_t len) {
    uint32_t at = lane;
    if (off < (len < 64u ? len : 64u)) at = (off & (off - 1u)) == 0u ? lane & (off - 1u) : lane % off;
    uint32_t left = len;
    while (left != 0u) {
      const uint32_t l = left < 64u ? left : 64u;
      uint8_t v = 0;
      if (lane < l) v = ring[(op - off + at) & (PAGE_RING - 1u)];
      __builtin_amdgcn_wave_barrier();
      if (lane < l) ring[(op + lane) & (PAGE_RING - 1u)] = v;
      __builtin_amdgcn_wave_barrier();
      op += l; left -= l;
      if (op - flushed >= 2u * PAGE_SEG) flush(false);
    }
  }
  // the page's end: the rest of the ring leaves for HBM, the verdict for status
  __device__ __forceinline__ void finish(uint32_t* verdict) {
    if (err == 0 && op != cap) err = 5;
    if (err == 0) flush(true);
    if (lane == 0) *verdict = err;
    __builtin_amdgcn_wave_barrier();
  }
};

__global__ __launch_bounds__(64) void snappy_decode_kernel(const uint8_t* __restrict__ src, const FdbCodecPage* __restrict__ pages, const int n_pages,
                                                           uint8_t* __restrict__ dst, uint32_t* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char smem[];
  for (int pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
    PageStream s(smem, src, dst, pages[pg]);
    // preamble: the uncompressed length as a varint
    {
      unsigned long long len = 0;
      const unsigned long long w = s.fetch(0);
      int shift = 0, k = 0;
      for (;; k++, shift += 7) {
        if ((uint32_t)k >= s.n || k >= 5) { s.err = 1; break; }
        const uint32_t b = (uint32_t)(w >> (8 * k)) & 0xFFu;
        len |= (unsigned long long)(b & 0x7Fu) << shift;
        if (!(b & 0x80u)) { k++; break; }
      }
      s.ip = (uint32_t)k;
      if (!s.err && len != (unsigned long long)s.cap) s.err = 1;
    }
    while (s.err == 0 && s.ip < s.n) {
      const unsigned long long w = s.fetch(s.ip);
      const uint32_t tag = (uint32_t)w & 0xFFu;
      if ((tag & 3u) == 0u) {  // literal
        uint32_t l = (tag >> 2) + 1u, hdr = 1u;
        if (l > 60u) {
          const uint32_t extra = l - 60u;  // 1 … 4 length bytes
          if (s.ip + 1u + extra > s.n) { s.err = 2; break; }
          l = (uint32_t)((w >> 8) & (extra == 4u ? 0xFFFFFFFFull : ((1ull << (8u * extra)) - 1ull))) + 1u;
          hdr = 1u + extra;
          if (l == 0u) { s.err = 2; break; }  // (2^32: more than a page can hold)
        }
        if ((unsigned long long)s.ip + hdr + l > s.n) { s.err = 2; break; }
        if ((unsigned long long)s.op + l > s.cap) { s.err = 3; break; }
        s.literals(s.ip + hdr, l);
        continue;
      }
      uint32_t l, off, hdr;
      if ((tag & 3u) == 1u) { hdr = 2u; l = 4u + ((tag >> 2) & 7u); off = ((tag >> 5) << 8) | ((uint32_t)(w >> 8) & 0xFFu); }
      else if ((tag & 3u) == 2u) { hdr = 3u; l = (tag >> 2) + 1u; off = (uint32_t)(w >> 8) & 0xFFFFu; }
      else { hdr = 5u; l = (tag >> 2) + 1u; off = (uint32_t)(w >> 8); }
      if (s.ip + hdr > s.n) { s.err = 2; break; }
      if (off == 0u || off > s.op) { s.err = 4; break; }
      if (off > FDB_PAGE_RING_REACH) { s.err = 6; break; }  // further back than the ring remembers (no compressor emits it)
      if ((unsigned long long)s.op + l > s.cap) { s.err = 3; break; }
      s.ip += hdr;
      s.match(off, l);  // l ≤ 64: one step
    }
    s.finish(status + pg);
  }
}

__global__ __launch_bounds__(64) void lz4_decode_kernel(const uint8_t* __restrict__ src, const FdbCodecPage* __restrict__ pages, const int n_pages,
                                                        uint8_t* __restrict__ dst, uint32_t* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char smem[];
  for (int pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
    PageStream s(smem, src, dst, pages[pg]);
    // a length's extension bytes at ip: added up to and including the first one ≠ 255, 64 of them per step — every lane looks at one,
    // a ballot finds the first that ends the run (a MiB of literals announces itself with ≈ 4 100 bytes of 0xFF: 65 steps, not 4 100).
    // Bytes past the stream's end read as 0, so a run that the stream cuts short ends there and is refused.
    auto extend = [&](unsigned long long& len) {
      for (;;) {
        if (!s.in_window(s.ip, 64u)) s.refill(s.ip);
        const uint32_t b = s.win[s.ip - s.base + s.lane];
        const unsigned long long stop = __builtin_amdgcn_ballot_w64(b != 255u);
        if (stop == 0ull) { len += 64u * 255u; s.ip += 64u; continue; }  // (64 bytes of the stream itself: ip stays ≤ n)
        const uint32_t f = (uint32_t)__builtin_ctzll(stop);
        if (f >= s.n - s.ip) { s.err = 2; return; }
        len += 255u * f + (uint32_t)__builtin_amdgcn_readlane((int)b, (int)f);
        s.ip += f + 1u;
        return;
      }
    };
    while (s.err == 0 && s.ip < s.n) {
      const unsigned long long w = s.fetch(s.ip);
      const uint32_t token = (uint32_t)w & 0xFFu;
      unsigned long long ll = token >> 4, ml = token & 15u;
      // (short literals: the offset behind them is in the 8 bytes already fetched)
      const bool off_in_w = ll <= 5ull;
      const uint32_t off_w = off_in_w ? (uint32_t)(w >> (8u * (1u + (uint32_t)ll))) & 0xFFFFu : 0u;
      s.ip += 1u;
      if (ll == 15ull) { extend(ll); if (s.err) break; }
      if (ll > (unsigned long long)(s.n - s.ip)) { s.err = 2; break; }
      if ((unsigned long long)s.op + ll > s.cap) { s.err = 3; break; }
      if (ll != 0ull) s.literals(s.ip, (uint32_t)ll);
      if (s.ip == s.n) break;  // the last sequence ends behind its literals
      if (s.n - s.ip < 2u) { s.err = 2; break; }
      const uint32_t off = off_in_w ? off_w : (uint32_t)s.fetch(s.ip) & 0xFFFFu;
      s.ip += 2u;
      if (ml == 15ull) { extend(ml); if (s.err) break; }
      ml += 4ull;
      if (off == 0u || off > s.op) { s.err = 4; break; }
      if (off > FDB_PAGE_RING_REACH) { s.err = 6; break; }  // further back than the ring remembers (the host takes such pages)
      if ((unsigned long long)s.op + ml > s.cap) { s.err = 3; break; }
      s.match(off, (uint32_t)ml);
    }
    s.finish(status + pg);
  }
}
}  // namespace

hipError_t fdb_launch_page_decode(int codec, const uint8_t* src, const FdbCodecPage* pages, int32_t n_pages, uint8_t* dst, uint32_t* status, hipStream_t stream) {
  if (codec != FDB_CODEC_SNAPPY && codec != FDB_CODEC_LZ4_RAW) return hipErrorInvalidValue;
  if (n_pages <= 0) return hipSuccess;
  const bool lz4 = codec == FDB_CODEC_LZ4_RAW;
  auto* const kernel = lz4 ? lz4_decode_kernel : snappy_decode_kernel;
  static bool attr_set[2] = {false, false};
  if (!attr_set[lz4]) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAGE_LDS); attr_set[lz4] = true; }
  hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int32_t>(n_pages, 8192)), dim3(64), PAGE_LDS, stream, src, pages, (int)n_pages, dst, status);
  return hipGetLastError();
}
