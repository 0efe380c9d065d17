// Host-only harness of the segment loader (lakeside_amd/csrc/loader.cpp): the Parquet walk, the dictionary
// interning and the staging copy, with no device upload, so it runs under ASan + UBSan and TSan on a machine without
// a GPU (`make sanitize`; VERDICT r4 next #8 -- the use-after-free of eebca43 was a ChunkOut stream pointing into a
// reallocated buffer, which ASan reports here).
//
//   load_check [--tiles[=<column>]] <threads> <file.parquet>...
//
// Loads every file in order into one set of engine dictionaries (as one engine would), stages each segment's stream
// area in three pieces (the piece boundaries of the upload path), and prints a digest per segment: rows, columns,
// unloaded columns, tiles, a hash of the staged bytes, of every column's pages / runs / tile columns / remap, and
// finally every dictionary's size and a hash of its values in id order.  The digest must not depend on the thread
// count (tests/test_load_check.py compares 1 and 8 threads).  A file that fails to load prints its error and the
// harness goes on (corrupt-file fixtures).
//
// --tiles: after each segment's digest, one line per tile for the `_cardinalhq.name` column -- what the name-clustered
// value copy's builder (Engine::build_cluster) and the scan kernels see of it: the tile's rows, TILE_TS_SORTED and
// ts_max - ts_min, the page kind, chunk dictionary size and index width, the first value index, the run count, and the
// first run's start and kind.  tests/test_clu_shapes_cpu.py pins its fixtures' shapes with it.  Without the flag the
// output is what it was.  --tiles=<column> prints the same lines for another column (tests/test_tag_shapes_cpu.py: the
// tag column the filter and group-dim decoders read); a segment without that column prints no tile line.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../include/lakeside_gpu.h"
#include "../lakeside_amd/csrc/loader.hpp"
#include "../lakeside_amd/csrc/plan.hpp"

using namespace lk;

namespace {
uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
constexpr uint64_t kFnv0 = 1469598103934665603ull;
}  // namespace

int main(int argc, char** argv) {
  bool show_tiles = false;
  std::string tile_col = "_cardinalhq.name";
  if (argc > 1 && !strncmp(argv[1], "--tiles", 7) && (argv[1][7] == 0 || argv[1][7] == '=')) {
    show_tiles = true;
    if (argv[1][7] == '=') tile_col = argv[1] + 8;
    argv++;
    argc--;
  }
  if (argc < 3) {
    fprintf(stderr, "usage: load_check [--tiles[=<column>]] <threads> <file.parquet>...\n");
    return 2;
  }
  const int threads = atoi(argv[1]);
  std::map<std::string, std::unique_ptr<GlobalDict>> dicts;
  std::mutex dicts_mu;
  auto dict = [&](const std::string& c) -> GlobalDict& {
    std::lock_guard<std::mutex> g(dicts_mu);
    auto& d = dicts[c];
    if (!d) d = std::make_unique<GlobalDict>();
    return *d;
  };
  int failures = 0;
  for (int a = 2; a < argc; a++) {
    std::ifstream f(argv[a], std::ios::binary);
    std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), {});
    const char* base = strrchr(argv[a], '/');
    base = base ? base + 1 : argv[a];
    try {
      HostLoad H = load_host(argv[a], bytes.data(), bytes.size(), threads, dict);
      const SegmentData& S = H.seg;
      fprintf(stderr, "%s: host load %.1f ms (%.2f GB/s of Parquet, %d threads)\n", base, H.host_ms,
              bytes.size() / (H.host_ms * 1e6), threads);
      std::vector<uint8_t> area(S.data_bytes, 0xA5);   // poisoned: every byte must be written by the staging
      StagePlan plan(H);
      const size_t piece = std::max<size_t>(size_t(1) << 12, (S.data_bytes + 2) / 3);
      for (size_t lo = 0; lo < S.data_bytes; lo += piece) {
        const size_t hi = std::min(S.data_bytes, lo + piece);
        std::vector<uint8_t> pin(hi - lo, 0x5A);
        plan.stage(pin.data(), lo, hi, threads);
        memcpy(area.data() + lo, pin.data(), hi - lo);
      }
      printf("%s rows=%lld cols=%zu tiles=%zu data=%zu staged=%016llx\n", base, (long long)S.num_rows, S.cols.size(),
             S.tiles.size(), S.data_bytes, (unsigned long long)fnv(kFnv0, area.data(), area.size()));
      for (auto& u : S.unloaded) printf("  unloaded %s: %s\n", u.first.c_str(), u.second.c_str());
      printf("  tiles %016llx\n", (unsigned long long)fnv(kFnv0, S.tiles.data(), S.tiles.size() * sizeof(TileDesc)));
      for (const HostCol& c : S.cols) {
        uint64_t h = fnv(kFnv0, c.pages.data(), c.pages.size() * sizeof(PageDesc));
        h = fnv(h, c.runs.data(), c.runs.size() * sizeof(RunDesc));
        h = fnv(h, c.tcols.data(), c.tcols.size() * sizeof(TileCol));
        h = fnv(h, c.remap.data(), c.remap.size() * sizeof(uint32_t));
        printf("  col %s type=%d pages=%zu runs=%zu remap=%zu %016llx\n", c.name.c_str(), c.ptype, c.pages.size(),
               c.runs.size(), c.remap.size(), (unsigned long long)h);
      }
      const int cn = show_tiles ? S.col_index(tile_col) : -1;
      if (cn >= 0 && S.cols[size_t(cn)].tcols.size() == S.tiles.size()) {
        const HostCol& N = S.cols[size_t(cn)];
        for (size_t t = 0; t < S.tiles.size(); t++) {
          const TileDesc& td = S.tiles[t];
          const TileCol& tc = N.tcols[t];
          const bool run0 = tc.nruns > 0 && size_t(tc.run_lo) < N.runs.size();
          const RunDesc r0 = run0 ? N.runs[tc.run_lo] : RunDesc{0u, 0u, 0u, 0u};
          printf("  tile %zu rg=%u nrows=%u sorted=%u span=%lld kind=%u dict_n=%u bw=%u vbase=%u nruns=%u has_nulls=%u "
                 "run0_start=%u run0_lit=%u\n",
                 t, td.rg, td.nrows, td.pad & TILE_TS_SORTED, (long long)(td.ts_max - td.ts_min), unsigned(tc.kind),
                 tc.dict_n, unsigned(tc.bw), tc.vbase, tc.nruns, unsigned(tc.has_nulls), r0.start, r0.off_lit >> 31);
        }
      }
    } catch (const PlanError& e) {
      printf("%s error %d: %s\n", base, e.code, e.what());
      failures++;
    } catch (const std::exception& e) {
      printf("%s error: %s\n", base, e.what());
      failures++;
    }
  }
  for (auto& kv : dicts) {
    const GlobalDict& d = *kv.second;
    uint64_t h = kFnv0;
    for (size_t i = 0; i < d.size(); i++) {
      h = fnv(h, d[i].data(), d[i].size());
      h = fnv(h, "\0", 1);
      if (d.ids.find(d[i]) != i) {
        printf("dict %s: value %zu is not indexed under its id\n", kv.first.c_str(), i);
        return 1;
      }
    }
    printf("dict %s size=%zu refs=%zu %016llx\n", kv.first.c_str(), d.size(), d.refs.size(), (unsigned long long)h);
  }
  printf("failures=%d\n", failures);
  return 0;
}
