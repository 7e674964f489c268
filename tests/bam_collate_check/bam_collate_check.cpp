// TEST INFRASTRUCTURE ONLY: the collation of BAM input (csrc/fq_bamin.h (b'), csrc/fq_frontend.cpp) under AddressSanitizer / UBSan, linked against the host-loop build of
// the library.  Runs the corpus tests/test_bam_collate.py wrote -- the kernel-entry cases, the refusals, the seeded stream, each with what the test's own walk and transcoder
// made of it: pairs, orphans, the first refusal, the two texts -- through fq_bam_collate_device, as one chunk and as chunks of one 300-byte member each, with the hash's
// grouping bits unset and 0; then one BAM file of several chunks through fq_frontend_open_bam_collate, fetching every batch.
//     bam_collate_check <corpus file> <stream.bam> <batch pairs> <chunk pairs>
// Exit code 0 and "ok: N cases, P pairs, O orphans" when nothing differs (and the sanitizers found nothing).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "fastquick_amd.h"

static bool same(const void *a, const void *b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }
template <class T> static T take(const std::string &s, size_t &at) { T v; memcpy(&v, s.data() + at, sizeof v); at += sizeof v; return v; }

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: bam_collate_check <corpus file> <stream.bam> <batch pairs> <chunk pairs>\n"); return 2; }
  std::ifstream in(argv[1], std::ios_base::binary);
  const std::string c((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t at = 0;
  const uint32_t n_cases = take<uint32_t>(c, at);
  long bad = 0;
  for (uint32_t k = 0; k < n_cases; ++k) {
    const int32_t n_ref = take<int32_t>(c, at);
    const int64_t first = take<int64_t>(c, at), n_pay = take<int64_t>(c, at);
    const std::vector<uint8_t> pay(c.begin() + (long)at, c.begin() + (long)(at + (size_t)n_pay));      // (the library's test entry allocates payloads and texts to the byte, so a kernel body's access behind either is seen)
    at += (size_t)n_pay;
    const int64_t bad_rec = take<int64_t>(c, at);
    const int32_t bad_kind = take<int32_t>(c, at);
    const int64_t pairs = take<int64_t>(c, at), orphans = take<int64_t>(c, at), n1 = take<int64_t>(c, at), n2 = take<int64_t>(c, at);
    const std::string t1 = c.substr(at, (size_t)n1), t2 = c.substr(at + (size_t)n1, (size_t)n2);
    at += (size_t)(n1 + n2);
    std::vector<int64_t> cuts;
    for (int64_t o = 0; o < n_pay; o += 300) cuts.push_back(o);
    for (int bits = 0; bits < 2; ++bits) {
      if (bits) setenv("FASTQUICK_BAM_HASH_BITS", "0", 1); else unsetenv("FASTQUICK_BAM_HASH_BITS");
      for (int64_t per = 0; per < 2; ++per) {
        const size_t cap = 2 * pay.size() + 64;      // (a refused stream writes the texts of the chunks in front of the refusal)
        std::vector<uint8_t> o1(cap), o2(cap);
        fq_bam_collate_t r;
        const int rc = fq_bam_collate_device(0, pay.data(), pay.size(), cuts.data(), (int64_t)cuts.size(), per, n_ref, first, -1, (int64_t)1 << 30, o1.data(), cap, o2.data(), cap, &r);
        bool ok = rc == FQ_OK && r.bad_record == bad_rec && r.bad_kind == bad_kind;
        if (ok && bad_rec < 0) ok = r.pairs == pairs && (!r.paired || r.orphans == orphans) && r.text_len[0] == n1 && r.text_len[1] == n2 && same(o1.data(), t1.data(), (size_t)n1) && same(o2.data(), t2.data(), (size_t)n2);
        if (!ok) { fprintf(stderr, "case %u differs (bits %d, per %lld: rc %d, %lld pairs, %lld orphans, refusal %lld/%d)\n", k, bits, (long long)per, rc, (long long)r.pairs, (long long)r.orphans, (long long)r.bad_record, r.bad_kind); ++bad; }
      }
    }
  }
  unsetenv("FASTQUICK_BAM_HASH_BITS");
  // one stream of several chunks
  fq_frontend_t *fe = nullptr;
  if (fq_frontend_open_bam_collate(0, argv[2], atoi(argv[3]), atoll(argv[4]), 0, 160, (int64_t)1 << 30, &fe)) { fprintf(stderr, "fq_frontend_open_bam_collate failed\n"); return 1; }
  long long pairs = 0;
  for (;;) {
    fq_text_batch_t *b = nullptr;
    const int64_t n = fq_frontend_next(fe, &b);
    if (n < 0) { fprintf(stderr, "fq_frontend_next: %lld (%s)\n", (long long)n, fq_frontend_last_error(fe)); ++bad; break; }
    if (n == 0) break;
    const size_t rows = (size_t)n * 2;
    std::vector<uint64_t> head(3 * rows);
    std::vector<uint16_t> len(rows);
    std::vector<char> names(rows * 304);
    if (fq_text_batch_fetch(fe, b, head.data(), len.data(), names.data(), (int64_t)names.size()) < 0) ++bad;
    for (size_t i = 0; i < rows; ++i) if (len[i] != 100) { ++bad; break; }
    pairs += n;
    fq_frontend_release(fe, b);
  }
  fq_frontend_stats_t st;
  fq_frontend_stats(fe, &st);
  if (st.chunks < 3 || st.bam_records < 2 * pairs || st.bam_held_peak_records < st.bam_orphans) ++bad;
  fq_frontend_close(fe);
  if (bad) { fprintf(stderr, "%ld differences\n", bad); return 1; }
  printf("ok: %u cases, %lld pairs, %lld orphans\n", n_cases, pairs, (long long)st.bam_orphans);
  return 0;
}
