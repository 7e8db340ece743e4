// fdb_jit.cpp — plan-specialised scan kernels, compiled at run time with hiprtc: the source fdb_jitgen.cpp writes for a shape goes
// through the process cache (keyed by the shape), the disk cache (keyed by the source text) and the compiler, and is launched from here.
//
// Failure to compile (hiprtc missing, unexpected shape) is not an error: the caller falls back to the interpreting
// kernels — still on the GPU.
#include <hip/hip_runtime_api.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "fdb_jit.h"
#include "../../include/frostdb_amd.h"

namespace fdb {

namespace {

// The argument-block definitions the generated kernel shares with the host (fdb_kernels.h, embedded at build time).
const char* kKernelsHeader =
#include "fdb_kernels_h.inc"
    ;

// device | shape key → function. An entry is published BEFORE it is built: the thread that created it builds it (disk load or hiprtc,
// 130–500 ms) without holding g_mu, threads that want the same kernel wait for that entry alone, and everybody else's lookups go
// straight through. (Until round 6 the build ran under g_mu: while one chain compiled a new shape, every other query of the process —
// cached shapes too — stood still for the length of a compilation.)
struct KernelEntry {
  std::mutex m;
  std::condition_variable cv;
  bool ready = false;
  hipFunction_t fn = nullptr;
};
std::mutex g_mu;
std::unordered_map<std::string, std::shared_ptr<KernelEntry>> g_cache;
bool g_disabled = false;

uint64_t fnv(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
  return h;
}

// Directory of the on-disk code-object cache, or "" when there is none that can be trusted: cached .hsaco files are loaded as GPU
// code, so the directory must be a real directory (not a symlink) owned by this user and closed to everybody else — another
// local user must not be able to plant code objects under a predictable name. $FDB_JIT_CACHE, else $XDG_CACHE_HOME/frostdb_amd,
// else ~/.cache/frostdb_amd, else /tmp/frostdb_amd_jit_<uid> (all subject to the same check).
std::string cache_dir() {
  std::string d;
  if (const char* e = std::getenv("FDB_JIT_CACHE")) d = e;
  else if (const char* x = std::getenv("XDG_CACHE_HOME"); x != nullptr && *x) d = std::string(x) + "/frostdb_amd";
  else if (const char* h = std::getenv("HOME"); h != nullptr && *h) { ::mkdir((std::string(h) + "/.cache").c_str(), 0700); d = std::string(h) + "/.cache/frostdb_amd"; }
  else d = "/tmp/frostdb_amd_jit_" + std::to_string((long)getuid());
  if (d.empty()) return "";
  (void)::mkdir(d.c_str(), 0700);
  struct stat st;
  if (::lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != getuid() || (st.st_mode & 077) != 0) {
    static bool warned = false;
    if (!warned) { warned = true; std::fprintf(stderr, "[frostdb_amd] JIT disk cache disabled: %s is not a private directory of this user\n", d.c_str()); }
    return "";
  }
  return d;
}

bool compile(const std::string& src, std::vector<char>* code, std::string* log) {
  hiprtcProgram prog;
  const char* hdr_names[] = {"fdb_kernels.h"};
  const char* hdr_src[] = {kKernelsHeader};
  if (hiprtcCreateProgram(&prog, src.c_str(), "fdb_plan_kernel.hip", 1, hdr_src, hdr_names) != HIPRTC_SUCCESS) { *log = "hiprtcCreateProgram failed"; return false; }
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DFDB_DEVICE_ONLY=1"};
  const hiprtcResult r = hiprtcCompileProgram(prog, 5, opts);
  size_t n = 0;
  hiprtcGetProgramLogSize(prog, &n);
  if (n > 1) { log->resize(n); hiprtcGetProgramLog(prog, &(*log)[0]); }
  if (r != HIPRTC_SUCCESS) { hiprtcDestroyProgram(&prog); return false; }
  size_t sz = 0;
  hiprtcGetCodeSize(prog, &sz);
  code->resize(sz);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  return true;
}

}  // namespace

int jit_blocks_per_cu(hipFunction_t fn, int block, size_t lds_bytes) {
  int occ = 0;
  if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, block, lds_bytes) != hipSuccess || occ < 1) { (void)hipGetLastError(); occ = 1; }
  if (occ > 2048 / block) occ = 2048 / block;
  return occ;
}

namespace {
// Process cache → disk cache → hiprtc; `key` identifies the shape, `make_source` is only called on a process-cache miss.
std::atomic<int64_t> g_stat_compiled{0}, g_stat_compile_us{0}, g_stat_disk_loads{0};

// Disk cache → hiprtc → module, for the entry its caller owns; whatever happens the entry is completed (a waiter must not wait for
// ever — a failed build publishes nullptr = "interpret").
hipFunction_t build_kernel(KernelEntry* entry, const std::string& kernel_name_s, const std::string& src) {
  const char* kernel_name = kernel_name_s.c_str();
  struct Publish {
    KernelEntry* e; hipFunction_t fn = nullptr;
    ~Publish() { { std::lock_guard<std::mutex> lk(e->m); e->fn = fn; e->ready = true; } e->cv.notify_all(); }
  } publish{entry};
  std::vector<char> code;
  char name[64];
  std::snprintf(name, sizeof name, "/k_%016llx_%zu.hsaco", (unsigned long long)(fnv(src) ^ (fnv(kKernelsHeader) * 31)), src.size());
  const std::string dir = cache_dir();
  const std::string path = dir.empty() ? std::string() : dir + name;
  bool from_disk = false;
  if (!path.empty()) {
    std::ifstream f(path, std::ios::binary);
    if (f) code.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    from_disk = !code.empty();
  }
  auto load = [&](hipFunction_t* fn) {
    hipModule_t mod = nullptr;
    *fn = nullptr;
    if (hipModuleLoadData(&mod, code.data()) == hipSuccess && hipModuleGetFunction(fn, mod, kernel_name) == hipSuccess) return true;
    (void)hipGetLastError();
    *fn = nullptr;
    return false;
  };
  hipFunction_t fn = nullptr;
  if (from_disk && !load(&fn)) {  // truncated / stale / foreign file: drop it and compile afresh instead of living on the fallback forever
    (void)::unlink(path.c_str());
    code.clear();
    from_disk = false;
  }
  if (from_disk) g_stat_disk_loads++;
  if (code.empty()) {
    std::string log;
    bool compiled;
    {
      // (one compilation at a time: the compiler is not known to tolerate concurrent programs, and lookups no longer wait behind it)
      static std::mutex compile_mu;
      std::lock_guard<std::mutex> lk(compile_mu);
      const auto t0 = std::chrono::steady_clock::now();
      compiled = compile(src, &code, &log);
      g_stat_compile_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    g_stat_compiled++;
    if (!compiled) {
      std::fprintf(stderr, "[frostdb_amd] %s specialisation failed, using the interpreting kernel: %s\n", kernel_name, log.c_str());
      if (std::getenv("FDB_JIT_DEBUG")) std::fprintf(stderr, "%s\n", src.c_str());
      return nullptr;
    }
    if (!path.empty()) {  // publish atomically, and only a file that was written completely
      const std::string tmp = path + "." + std::to_string((long)getpid());
      bool ok = false;
      {
        std::ofstream f(tmp, std::ios::binary);
        if (f) { f.write(code.data(), (std::streamsize)code.size()); f.close(); ok = !f.fail(); }
      }
      if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) (void)::unlink(tmp.c_str());
    }
  }
  if (fn == nullptr && !load(&fn)) {
    std::fprintf(stderr, "[frostdb_amd] could not load a specialised %s, using the interpreting kernel\n", kernel_name);
    fn = nullptr;
  }
  publish.fn = fn;
  return fn;
}

// $FDB_JIT_ASYNC=1 (opt-in): a caller that CAN do without the specialised kernel (jit_may_defer: the interpreting kernels serve its
// launch) does not wait for a kernel that has to be built first — the build runs on a thread of this pool, the call returns nullptr
// ("interpret"), and the next query of the shape finds the kernel. The first query of a new shape then costs an interpreted scan
// instead of 130–500 ms of compiler. The threads are joined before the cache they publish into is destroyed.
thread_local bool t_may_defer = false;
struct Builders {
  struct Slot { std::thread t; std::shared_ptr<std::atomic<bool>> done; };
  std::mutex m;
  std::vector<Slot> slots;
  void spawn(std::function<void()> job) {
    std::lock_guard<std::mutex> lk(m);
    // (threads that have finished are joined here: an unjoined thread keeps its stack, and a long-lived process meets many shapes)
    for (size_t k = 0; k < slots.size();) {
      if (slots[k].done->load(std::memory_order_acquire)) { slots[k].t.join(); slots[k] = std::move(slots.back()); slots.pop_back(); }
      else k++;
    }
    auto done = std::make_shared<std::atomic<bool>>(false);
    slots.push_back(Slot{std::thread([job = std::move(job), done] { job(); done->store(true, std::memory_order_release); }), done});
  }
  ~Builders() { for (Slot& s : slots) if (s.t.joinable()) s.t.join(); }
} g_builders;

template <typename F>
hipFunction_t get_kernel(const std::string& key, const char* kernel_name, F make_source) {
  if (g_disabled || std::getenv("FDB_NO_JIT") != nullptr) return nullptr;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const std::string ckey = std::to_string(dev) + "|" + kernel_name + "|" + key;  // a loaded module belongs to one device
  std::shared_ptr<KernelEntry> entry;
  bool builder = false;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_cache.find(ckey);
    if (it == g_cache.end()) { entry = std::make_shared<KernelEntry>(); g_cache.emplace(ckey, entry); builder = true; }
    else entry = it->second;
  }
  const char* as = t_may_defer ? std::getenv("FDB_JIT_ASYNC") : nullptr;
  const bool defer = as != nullptr && std::atoi(as) != 0;
  if (!builder) {
    std::unique_lock<std::mutex> lk(entry->m);
    if (defer && !entry->ready) return nullptr;  // still being built: this launch is interpreted
    entry->cv.wait(lk, [&] { return entry->ready; });
    return entry->fn;
  }
  std::string src;
  try { src = make_source(); }
  catch (...) { { std::lock_guard<std::mutex> lk(entry->m); entry->ready = true; } entry->cv.notify_all(); throw; }
  if (defer) {
    const std::string kn = kernel_name;
    g_builders.spawn([entry, kn, src, dev] { (void)hipSetDevice(dev); (void)build_kernel(entry.get(), kn, src); });
    return nullptr;
  }
  return build_kernel(entry.get(), kernel_name, src);
}
}  // namespace

hipFunction_t jit_select_kernel_get(const JitShape& shape) {
  return get_kernel("select|" + shape.key() + "|f" + std::to_string(shape.fuse4) + "," + std::to_string(shape.fuse8), "fdb_select_kernel", [&] { return jit_select_source(shape); });
}
hipError_t jit_select_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_super_tiles, const FdbScanArgs& common, int grid, size_t lds_bytes,
                             uint32_t* masks, uint32_t* offsets, const FdbSelectArgs& sel, hipStream_t stream) {
  long long tt = total_super_tiles;
  void* args[] = {(void*)&d_parts, (void*)&n_parts, (void*)&tt, (void*)&common, (void*)&masks, (void*)&offsets, (void*)&sel};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, (unsigned)jit_select_block(), 1, 1, (unsigned)lds_bytes, stream, args, nullptr);
}

hipFunction_t jit_flags_get(const JitShape& shape) {
  return get_kernel("flags|" + shape.key(), "fdb_flags_kernel", [&] { return jit_flags_source(shape); });
}

hipError_t jit_flags_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_super_tiles, const FdbScanArgs& common, int grid, size_t lds_bytes,
                            uint32_t* masks, uint32_t* tile_counts, hipStream_t stream) {
  long long tt = total_super_tiles;
  void* args[] = {(void*)&d_parts, (void*)&n_parts, (void*)&tt, (void*)&common, (void*)&masks, (void*)&tile_counts};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, 256u, 1, 1, (unsigned)lds_bytes, stream, args, nullptr);
}

hipFunction_t jit_project_get(const JitShape& shape) {
  std::string roots;
  for (int r : shape.proj_roots) roots += std::to_string(r) + ",";
  return get_kernel("project|" + shape.key() + "|r" + roots, "fdb_project_kernel", [&] { return jit_project_source(shape); });
}
hipError_t jit_project_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_tiles, int grid, size_t lds_bytes, const FdbProjectPart* d_outs,
                              unsigned long long* d_nulls, hipStream_t stream) {
  long long tt = total_tiles;
  void* args[] = {(void*)&d_parts, (void*)&n_parts, (void*)&tt, (void*)&d_outs, (void*)&d_nulls};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, 256u, 1, 1, (unsigned)lds_bytes, stream, args, nullptr);
}

void jit_stats(int64_t* n_compiled, double* compile_ms, int64_t* n_disk_loads) {
  if (n_compiled) *n_compiled = g_stat_compiled.load();
  if (compile_ms) *compile_ms = (double)g_stat_compile_us.load() / 1000.0;
  if (n_disk_loads) *n_disk_loads = g_stat_disk_loads.load();
}

JitDeferScope::JitDeferScope(bool may_defer) : prev_(t_may_defer) { t_may_defer = may_defer; }
JitDeferScope::~JitDeferScope() { t_may_defer = prev_; }

hipFunction_t jit_get(const JitShape& shape) {
  return get_kernel(shape.key(), "fdb_plan_kernel", [&] { return jit_source(shape); });
}

hipFunction_t jit_hash_get(const JitHashShape& shape) {
  return get_kernel(shape.key(), "fdb_hash_kernel", [&] { return jit_hash_source(shape); });
}

hipError_t jit_hash_launch(hipFunction_t fn, const FdbHashArgs& args, int grid, size_t lds_bytes, hipStream_t stream) {
  void* kargs[] = {(void*)&args};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, 256, 1, 1, (unsigned)lds_bytes, stream, kargs, nullptr);
}

// Geometry for `shape`. Measured on MI355X (tools/sweep_geometry.sh): a streaming scan is fastest when ≈64 KB of loads
// are in flight per CU (Little's law for ≈8 TB/s × ≈2 µs over 256 CUs) — 16 waves for cfg 2 (64 B per lane and tile),
// 8 for cfg 3 (128 B) — and gets SLOWER with more resident waves (cfg 2: 6.75 TB/s at 16 waves/CU, 6.0 at 32), so the
// persistent grid is sized from the bytes one lane requests per tile, not from the occupancy limit.
hipFunction_t jit_select(JitShape shape, size_t lds_bytes, int row_bytes, bool sorted_input, int* block_out, int* blocks_per_cu_out) {
  int waves = row_bytes > 0 ? (65536 / (64 * 4)) / row_bytes : 16;  // 64 lanes × 4 rows per lane and tile
  waves = std::max(8, std::min(32, waves));
  // A quad shape (JitShape::quad) keeps four sub-steps in flight per wave, 16 rows per lane, all of a block's early loads issued before
  // its first branch (Gen::block_loads), and is fastest with ≈96 KB in flight per CU in 256-thread workgroups, at least two of them
  // (profiles/block_loads_ab.json, "geometry": 2 per CU for the headline's 11 B per row — 3, 4 and 6 are slower, as are 1 024-thread
  // workgroups —, 2 per CU for cfg 3's 20 B per row). While the optimiser still sank sub-step 0's loads below that branch a wave had
  // 2 KiB in flight for half of a block's time, and 3 per CU were the best (profiles/quad_scan_ab.json).
  // An ordered plan's input is sorted by its group columns: every wave takes the uniform fold, whose butterflies are a long dependent
  // chain behind each sub-step, and wants the third workgroup to load meanwhile (cfg 2 sorted: 0.197 ms per 100 M rows at 3 per CU,
  // 0.238 at 2).
  // The packed index forms (fdb_record.h) take the headline's row from 11 to 10 B: unordered it stays at 2 per CU (3 again slower, 1.749
  // against 1.605 ms per step in three pairs), but 144 / 10 would give the ordered plan 4 per CU, which loses what the saved byte wins
  // (cfg 2 sorted at 10 B per row: 0.257 ms per step at 3 per CU, 0.271 at 4, every one of three pairs; profiles/packed_index_ab.json) —
  // so an ordered quad launch takes at most 12 waves, 3 per CU, the one count measured best on both sides.
  if (shape.quad) waves = std::max(8, std::min(sorted_input ? 12 : 16, row_bytes > 0 ? (sorted_input ? 144 : 96) / row_bytes : 8));
  const int block = shape.quad ? 256 : waves % 8 == 0 ? 512 : 256;
  shape.block = block;
  hipFunction_t fn = jit_get(shape);
  if (fn == nullptr) return nullptr;
  const int fit = jit_blocks_per_cu(fn, block, lds_bytes);
  *block_out = block;
  *blocks_per_cu_out = std::max(1, std::min(fit, (waves + block / 128) / (block / 64)));
  if (std::getenv("FDB_JIT_DEBUG"))
    std::fprintf(stderr, "[frostdb_amd] plan kernel %s: %d B/row, %zu B LDS -> %d-thread workgroups, %d per CU (%d fit)\n", shape.key().c_str(), row_bytes,
                 lds_bytes, block, *blocks_per_cu_out, fit);
  return fn;
}

hipError_t jit_launch(hipFunction_t fn, const FdbScanArgs* d_parts, int n_parts, int64_t total_tiles, const FdbScanArgs& common, int grid, int block,
                      size_t lds_bytes, hipStream_t stream) {
  long long tt = total_tiles;
  void* args[] = {(void*)&d_parts, (void*)&n_parts, (void*)&tt, (void*)&common};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, (unsigned)block, 1, 1, (unsigned)lds_bytes, stream, args, nullptr);
}

hipError_t jit_launch_ptab(hipFunction_t fn, const unsigned long long* d_ptab, int n_parts, int64_t total_tiles, const FdbScanArgs& common, int grid, int block,
                           size_t lds_bytes, hipStream_t stream) {
  long long tt = total_tiles;
  void* args[] = {(void*)&d_ptab, (void*)&n_parts, (void*)&tt, (void*)&common};
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, (unsigned)block, 1, 1, (unsigned)lds_bytes, stream, args, nullptr);
}

}  // namespace fdb
