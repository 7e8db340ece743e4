// CPU-only: prints what the host-side decisions of a dense scan launch (frostdb_amd/csrc/fdb_launch_plan.h, LutClasses of
// fdb_plan_internal.h) give for inputs on the command line, so that tests/test_launch_plan_cpu.py can hold them to hand-worked values.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I frostdb_amd/csrc -I include -I /opt/rocm/include tools/launch_plan_dump.cpp frostdb_amd/csrc/*.o \
//       -L/opt/rocm/lib -lamdhip64 -lhiprtc -ldl -lpthread -lz -Wl,-rpath,/opt/rocm/lib -o /tmp/launch_plan_dump
//   lds <lut_lds_max> <acc_bytes> <n_aggs> <jit_possible> <slots_ok> <fixed_order> <use_partials> <grid_override> <base_grid>
//   tiles <tile_rows> <rows> …        one record per row count, in launch order
//   funcs <func>:<type> …             fdb_agg_func : FdbAggType per aggregation
//   luts <hex bytes | -> …            one record per argument: its one LUT as hex, `-`: a record without LUTs
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <vector>

#include "fdb_launch_plan.h"
#include "fdb_plan_internal.h"

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "lds" && argc == 11) {
    auto v = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
    const fdb::LdsPlan p = fdb::plan_lds(v(2), v(3), v(4), v(5) != 0, v(6) != 0, v(7) != 0, v(8) != 0, (int)v(9), (int)v(10));
    std::printf("lds_acc=%d lds_bytes=%zu cache_slots=%d base_grid=%d refusal=%s\n", p.lds_acc, p.lds_bytes, p.cache_slots, p.base_grid, p.refusal.c_str());
    return 0;
  }
  if (mode == "tiles" && argc >= 3) {
    std::vector<FdbScanArgs> parts((size_t)argc - 3);
    for (size_t k = 0; k < parts.size(); k++) parts[k].n_rows = std::atoll(argv[3 + k]);
    const int64_t total = fdb::assign_tiles(parts.data(), parts.size(), std::atoll(argv[2]));
    for (const FdbScanArgs& a : parts) std::printf("%lld %lld\n", (long long)a.tile_begin, (long long)a.tile_end);
    std::printf("total=%lld\n", (long long)total);
    return 0;
  }
  if (mode == "funcs") {
    std::vector<int32_t> func, type;
    for (int i = 2; i < argc; i++) { int f = 0, t = 0; if (std::sscanf(argv[i], "%d:%d", &f, &t) != 2) return 2; func.push_back(f); type.push_back(t); }
    const fdb::FoldFuncs F = fdb::fold_funcs(func.data(), type.data(), func.size());
    for (size_t j = 0; j < 1 + func.size(); j++) std::printf("%d%c", F.f[j], j == func.size() ? '\n' : ' ');
    return 0;
  }
  if (mode == "luts") {
    std::deque<fdb::Plan::Resolved> Rs;  // (LutClasses keeps pointers to its records)
    fdb::LutClasses L;
    for (int i = 2; i < argc; i++) {
      Rs.emplace_back();
      const std::string hex = argv[i];
      if (hex != "-") {
        std::vector<uint8_t> bytes;
        for (size_t c = 0; c + 1 < hex.size(); c += 2) bytes.push_back((uint8_t)std::strtoul(hex.substr(c, 2).c_str(), nullptr, 16));
        const size_t off = Rs.back().blob.add(bytes.data(), bytes.size());
        Rs.back().luts.push_back(fdb::PendingLut{0, 0, off, bytes.size()});
      }
      L.add(Rs.back());
    }
    for (size_t k = 0; k < Rs.size(); k++) std::printf("class=%d blob_base=%zu\n", L.cls[k], L.blob_base[k]);
    std::printf("blob=%zu\n", L.blob.bytes.size());
    return 0;
  }
  std::fprintf(stderr, "launch_plan_dump: lds | tiles | funcs | luts (see the head of tools/launch_plan_dump.cpp)\n");
  return 2;
}
