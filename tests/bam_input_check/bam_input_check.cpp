// TEST INFRASTRUCTURE ONLY: BAM input (csrc/fq_bamin.h, csrc/fq_frontend.cpp) under AddressSanitizer / UBSan, linked against the host-loop build of the library.
// Runs a corpus of payloads that tests/test_bam_input.py wrote (the entry corpus, one record set cut at every byte, decoys at member starts with the repairs they must take, the
// refusals) -- each with its member cuts and with what the test's own transcoder made of it: record starts, the
// two texts, the first refusal -- through fq_bam_transcode_device and compares; then one BAM file of several chunks through fq_frontend_open_bam, fetching every batch.
//     bam_input_check <corpus file> <stream.bam> <batch pairs> <chunk pairs>
// Exit code 0 and "ok: N cases, P pairs" when nothing differs (and the sanitizers found nothing).
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
  if (argc != 5) { fprintf(stderr, "usage: bam_input_check <corpus file> <stream.bam> <batch pairs> <chunk pairs>\n"); return 2; }
  std::ifstream in(argv[1], std::ios_base::binary);
  const std::string c((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t at = 0;
  const uint32_t n_cases = take<uint32_t>(c, at);
  long bad = 0;
  for (uint32_t k = 0; k < n_cases; ++k) {
    const int32_t n_ref = take<int32_t>(c, at);
    const int64_t first = take<int64_t>(c, at), n_pay = take<int64_t>(c, at);
    const uint32_t n_cuts = take<uint32_t>(c, at);
    const std::vector<uint8_t> pay(c.begin() + (long)at, c.begin() + (long)(at + (size_t)n_pay));      // (the library's test entry allocates payload and texts to the byte, so a kernel body's access behind either is seen)
    at += (size_t)n_pay;
    std::vector<int64_t> cuts(n_cuts);
    for (auto &x : cuts) x = take<int64_t>(c, at);
    const int64_t bad_rec = take<int64_t>(c, at);
    const int32_t bad_kind = take<int32_t>(c, at), least_repairs = take<int32_t>(c, at);
    const int64_t chain_end = take<int64_t>(c, at), carry_from = take<int64_t>(c, at);
    const int64_t n1 = take<int64_t>(c, at), n2 = take<int64_t>(c, at);
    const uint32_t n_starts = take<uint32_t>(c, at);
    const std::string t1 = c.substr(at, (size_t)n1), t2 = c.substr(at + (size_t)n1, (size_t)n2);
    at += (size_t)(n1 + n2);
    std::vector<uint32_t> starts(n_starts);
    for (auto &x : starts) x = take<uint32_t>(c, at);
    std::vector<uint8_t> o1((size_t)n1 + 1), o2((size_t)n2 + 1);
    std::vector<uint32_t> os(n_starts + 1);
    fq_bam_transcode_t r;
    const int rc = fq_bam_transcode_device(0, pay.data(), pay.size(), cuts.data(), (int64_t)cuts.size(), n_ref, first, -1, o1.data(), (size_t)n1, o2.data(), (size_t)n2, os.data(), n_starts, &r);
    bool ok = rc == FQ_OK && r.records == (int64_t)n_starts && r.bad_record == bad_rec && r.bad_kind == bad_kind && r.chain_repairs >= least_repairs && r.chain_end == chain_end && r.carry_from == carry_from && same(os.data(), starts.data(), 4 * (size_t)n_starts);
    if (ok && bad_rec < 0) ok = r.text_len[0] == n1 && r.text_len[1] == n2 && same(o1.data(), t1.data(), (size_t)n1) && same(o2.data(), t2.data(), (size_t)n2);
    if (!ok) { fprintf(stderr, "case %u differs (rc %d, %lld records, refusal %lld/%d, %d repairs of %d at least)\n", k, rc, (long long)r.records, (long long)r.bad_record, r.bad_kind, r.chain_repairs, least_repairs); ++bad; }
  }
  // one stream of several chunks
  fq_bam_probe_t pr;
  if (fq_bam_probe(argv[2], &pr)) { fprintf(stderr, "%s\n", pr.error); return 1; }
  fq_frontend_t *fe = nullptr;
  if (fq_frontend_open_bam(0, argv[2], atoi(argv[3]), atoll(argv[4]), 0, 160, &fe)) { fprintf(stderr, "fq_frontend_open_bam failed\n"); return 1; }
  long long pairs = 0;
  for (;;) {
    fq_text_batch_t *b = nullptr;
    const int64_t n = fq_frontend_next(fe, &b);
    if (n < 0) { fprintf(stderr, "fq_frontend_next: %lld (%s)\n", (long long)n, fq_frontend_last_error(fe)); ++bad; break; }
    if (n == 0) break;
    const size_t rows = (size_t)n * (pr.paired ? 2 : 1);
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
  if (st.chunks < 3 || st.bam_records < 2 * pairs) ++bad;
  fq_frontend_close(fe);
  if (bad) { fprintf(stderr, "%ld differences\n", bad); return 1; }
  printf("ok: %u cases, %lld pairs\n", n_cases, pairs);
  return 0;
}
