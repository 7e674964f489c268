// TEST INFRASTRUCTURE ONLY: the binned form of the packed filter (csrc/fq_kernels.h "the same filter, binned") as the host loops of fq_emu_binned.h (the
// ones the host-loop backend runs behind the tuning key: count and offsets, bin, probe bucket by bucket, verdict) against the direct statement fq_prep_packed_thread, which
// the CPU tier holds to the oracle: filtered[], sub_max, sub_whole and the counters must be equal for every case.  Cases: 1 .. 4,099 reads, thresholds
// 1, 2 (18 probes binned), 3, 5, 19, uniform and ragged lengths with trimming, keys drawn at random over bitmaps that hold a share of them, every key 0
// (bucket 0x00, offset 0) and every key 2^32 - 1 (bucket 0xff, offset 2^24 - 1), and one read repeated.  Exit code 0 and "ok" when nothing differs.
#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "fastquick_amd.h"
#include "fq_kernels.h"
#include "fq_emu_binned.h"

static long g_bad = 0;

struct Out {
  std::vector<uint8_t> filtered;
  std::vector<int32_t> sub;      // sub_max, then sub_whole
  std::vector<uint64_t> counters;
  bool operator==(const Out &o) const { return filtered == o.filtered && sub == o.sub && counters == o.counters; }
};

int main() {
  uint8_t *bitmap[6];
  for (auto &b : bitmap) {      // 512 MiB each, untouched pages stay unmapped zeros
    b = (uint8_t *)mmap(nullptr, (size_t)1 << 29, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (b == MAP_FAILED) { perror("mmap"); return 2; }
  }
  std::mt19937_64 rng(20261021);
  long &bad = g_bad; long cases = 0, passed = 0, rejected = 0;
  const int sizes[] = {1, 63, 64, 65, 257, 4099};
  const int threshs[] = {1, 2, 3, 5, 19};
  for (int kind = 0; kind < 4; ++kind)        // 0: random keys, 1: every k-mer all A, 2: every k-mer all T, 3: one read repeated
    for (int n : sizes)
      for (int th : threshs)
        for (int ragged = 0; ragged < 2; ++ragged) {
          if (kind != 0 && (n != 4099 && n != 65)) continue;
          std::vector<uint64_t> head((size_t)3 * n);
          for (auto &k : head) k = kind == 1 ? 0 : kind == 2 ? ~0ull : rng();
          if (kind == 3) for (int ch = 0; ch < 3; ++ch) for (int r = 1; r < n; ++r) head[(size_t)ch * n + r] = head[(size_t)ch * n];
          // a share of the probes' bits is set: about half of the reads of kind 0 see hits, a few of them on every probe
          std::vector<std::pair<int, uint32_t>> set;
          for (int r = 0; r < n; ++r) {
            const uint64_t kmer[3] = {head[r], head[(size_t)n + r], head[(size_t)2 * n + r]};
            const unsigned dice = (unsigned)(rng() % 8);
            for (int q = 0; q < 18; ++q)
              if (dice == 0 || (dice < 4 && rng() % 3 == 0)) set.push_back({q % 6, fq_filter_key(kmer, q)});
          }
          for (auto &s : set) bitmap[s.first][s.second >> 3] |= (uint8_t)(1u << (s.second & 7u));
          std::vector<uint16_t> len((size_t)n);
          std::vector<uint8_t> qual_last((size_t)n);
          for (int r = 0; r < n; ++r) { len[r] = (uint16_t)(10 + rng() % 140); qual_last[r] = (uint8_t)(33 + rng() % 40); }
          const int n_pairs = (n + 1) / 2, batch_pairs = 100, n_sub = (n_pairs + batch_pairs - 1) / batch_pairs;
          Out got[2];
          for (int form = 0; form < 2; ++form) {
            Out &o = got[form];
            o.filtered.assign((size_t)n, 0xee); o.sub.assign((size_t)2 * n_sub, 0); o.counters.assign(FQ_C_COUNT, 0);
            FqPrepPackedArgs a{};
            for (int t = 0; t < 6; ++t) a.ix.bitmap[t] = bitmap[t];
            a.o.filter_thresh = th; a.o.trim_qual = 15;
            a.head = head.data(); a.len = ragged ? len.data() : nullptr; a.uniform_len = 150; a.n_reads = n;
            a.qual_last = ragged ? qual_last.data() : nullptr;
            a.filtered = o.filtered.data(); a.sub_max = o.sub.data(); a.sub_whole = o.sub.data() + n_sub;
            a.n_pairs = n_pairs; a.batch_pairs = batch_pairs; a.counters = o.counters.data();
            if (form == 0) for (int r = 0; r < n; ++r) fq_prep_packed_thread(a, r);
            else g_bad += fq_emu_prep_packed_binned(a);
          }
          ++cases;
          if (!(got[0] == got[1])) { ++bad; printf("kind %d, %d reads, thresh %d, ragged %d: the two forms differ\n", kind, n, th, ragged); }
          for (uint8_t f : got[0].filtered) { if (f) ++rejected; else ++passed; }
          for (auto &s : set) bitmap[s.first][s.second >> 3] = 0;
        }
  if (!passed || !rejected) { printf("the cases hold only one verdict (%ld passed, %ld rejected)\n", passed, rejected); ++bad; }
  printf("%ld cases, %ld reads passed, %ld rejected, %ld differences\n", cases, passed, rejected, bad);
  if (!bad) printf("ok\n");
  return bad ? 1 : 0;
}
