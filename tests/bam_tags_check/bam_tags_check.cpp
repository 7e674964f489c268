// TEST INFRASTRUCTURE ONLY: BAM input by read group and with OQ qualities (csrc/fq_bamin.h (b''), csrc/fq_frontend.cpp: the _select entries) under AddressSanitizer / UBSan,
// linked against the host-loop build of the library.  Runs the corpus tests/test_bam_tags.py wrote -- payloads whose records carry every auxiliary type, decoys, fields
// no walk gets through, OQ values that fit and that do not, each with the IDs to select, the OQ flag and what the test's own walk and transcoder made of it --
// through fq_bam_transcode_device_select (one member, and members of 300 bytes; both fill forms) or fq_bam_collate_device_select (one chunk, and a chunk a member;
// the hash's grouping bits unset and 0); then one BAM file of several chunks through fq_frontend_open_bam_select, fetching every batch.
//     bam_tags_check <corpus file> <stream.bam> <batch pairs> <chunk pairs> <ID>...
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
  if (argc < 6) { fprintf(stderr, "usage: bam_tags_check <corpus file> <stream.bam> <batch pairs> <chunk pairs> <ID>...\n"); return 2; }
  std::ifstream in(argv[1], std::ios_base::binary);
  const std::string c((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  size_t at = 0;
  const uint32_t n_cases = take<uint32_t>(c, at);
  long bad = 0;
  for (uint32_t k = 0; k < n_cases; ++k) {
    const int32_t n_ids = take<int32_t>(c, at), n_blob = take<int32_t>(c, at), use_oq = take<int32_t>(c, at), collate = take<int32_t>(c, at);
    const int64_t n_pay = take<int64_t>(c, at);
    const std::string blob = c.substr(at, (size_t)n_blob);
    at += (size_t)n_blob;
    std::vector<const char *> ids;
    for (size_t p = 0; (int32_t)ids.size() < n_ids; p += strlen(blob.c_str() + p) + 1) ids.push_back(blob.c_str() + p);
    const std::vector<uint8_t> pay(c.begin() + (long)at, c.begin() + (long)(at + (size_t)n_pay));      // (the library's test entries allocate payloads and texts to the byte, so a kernel body's access behind either is seen)
    at += (size_t)n_pay;
    const int64_t bad_rec = take<int64_t>(c, at);
    const int32_t bad_kind = take<int32_t>(c, at);
    const int64_t units = take<int64_t>(c, at), unsel = take<int64_t>(c, at), n1 = take<int64_t>(c, at), n2 = take<int64_t>(c, at);
    const std::string t1 = c.substr(at, (size_t)n1), t2 = c.substr(at + (size_t)n1, (size_t)n2);
    at += (size_t)(n1 + n2);
    const fq_bam_select_t sel{ids.data(), n_ids, use_oq};
    std::vector<int64_t> cuts;
    for (int64_t o = 0; o < n_pay; o += 300) cuts.push_back(o);
    const int64_t zero = 0;
    const size_t cap = 2 * pay.size() + 64;
    for (int v = 0; v < 4; ++v) {      // (v & 1: members of 300 bytes / a chunk a member; v & 2: the other fill form / the hash masked to 0 bits)
      if (collate) { if (v & 2) setenv("FASTQUICK_BAM_HASH_BITS", "0", 1); else unsetenv("FASTQUICK_BAM_HASH_BITS"); }
      else { if (v & 2) setenv("FASTQUICK_BAM_FILL", "pieces", 1); else unsetenv("FASTQUICK_BAM_FILL"); }
      std::vector<uint8_t> o1(cap), o2(cap);
      fq_bam_tag_counts_t cnt;
      bool ok;
      long long got_units = 0, got_bad = 0;
      int got_kind = 0, rc;
      if (collate) {
        fq_bam_collate_t r;
        rc = fq_bam_collate_device_select(0, pay.data(), pay.size(), cuts.data(), (int64_t)cuts.size(), v & 1, 1, 0, -1, (int64_t)1 << 30, o1.data(), cap, o2.data(), cap, &sel, &cnt, &r);
        got_units = r.pairs; got_bad = r.bad_record; got_kind = r.bad_kind;
        ok = rc == FQ_OK && r.bad_record == bad_rec && r.bad_kind == bad_kind;
        if (ok && bad_rec < 0) ok = r.pairs == units && cnt.unselected == unsel && r.text_len[0] == n1 && r.text_len[1] == n2 && same(o1.data(), t1.data(), (size_t)n1) && same(o2.data(), t2.data(), (size_t)n2);
      } else {
        fq_bam_transcode_t r;
        rc = fq_bam_transcode_device_select(0, pay.data(), pay.size(), (v & 1) ? cuts.data() : &zero, (v & 1) ? (int64_t)cuts.size() : 1, 1, 0, -1, o1.data(), cap, o2.data(), cap, nullptr, 0, &sel, &cnt, &r);
        got_units = r.units; got_bad = r.bad_record; got_kind = r.bad_kind;
        ok = rc == FQ_OK && r.bad_record == bad_rec && r.bad_kind == bad_kind;
        if (ok && bad_rec < 0) ok = r.units == units && cnt.unselected == unsel && r.text_len[0] == n1 && r.text_len[1] == n2 && same(o1.data(), t1.data(), (size_t)n1) && same(o2.data(), t2.data(), (size_t)n2);
      }
      if (!ok) { fprintf(stderr, "case %u differs (variant %d, collate %d: rc %d, %lld units, refusal %lld/%d; wanted %lld units, %lld/%d)\n", k, v, collate, rc, got_units, got_bad, got_kind, (long long)units, (long long)bad_rec, bad_kind); ++bad; }
    }
  }
  unsetenv("FASTQUICK_BAM_HASH_BITS");
  unsetenv("FASTQUICK_BAM_FILL");
  // one stream of several chunks, selected and with OQ
  std::vector<const char *> ids(argv + 5, argv + argc);
  const fq_bam_select_t sel{ids.data(), (int32_t)ids.size(), 1};
  fq_bam_probe_t pr;
  if (fq_bam_probe_select(argv[2], &sel, &pr)) { fprintf(stderr, "fq_bam_probe_select: %s\n", pr.error); return 1; }
  fq_frontend_t *fe = nullptr;
  if (fq_frontend_open_bam_select(0, argv[2], atoi(argv[3]), atoll(argv[4]), 0, 160, &sel, &fe)) { fprintf(stderr, "fq_frontend_open_bam_select failed\n"); return 1; }
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
  if (st.chunks < 3 || !pr.paired || st.bam_unselected < 2 * pairs || st.bam_oq_records <= 0 || st.bam_oq_records > 2 * pairs) ++bad;
  fq_frontend_close(fe);
  char rg[256];
  int32_t n_rg = 0;
  int64_t rg_bytes = 0;
  if (fq_bam_read_groups(argv[2], rg, sizeof rg, &n_rg, &rg_bytes) || n_rg < (int32_t)ids.size()) ++bad;
  if (bad) { fprintf(stderr, "%ld differences\n", bad); return 1; }
  printf("ok: %u cases, %lld pairs\n", n_cases, pairs);
  return 0;
}
