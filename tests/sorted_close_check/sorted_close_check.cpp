// TEST INFRASTRUCTURE ONLY: the sorted BAM writer (csrc/fq_bam.cpp: fq_bam_create_sorted) under AddressSanitizer / UBSan, linked against the host-loop build of the
// library.  Aligns a FASTQ pair in batches on a context with a sorted writer attached (runs the call sorts, kept in memory) and hands the same records as bytes to a
// second sorted writer with sort_mem = 1 (entries from bytes, every run in a spill file, read back with pread) and to a third whose runs alternate between memory and
// files; a fourth is closed without a record.  The three closes -- key sort, run bookkeeping, assembly in slices, compression, the .bai builder -- must leave the same
// BAM file and the same index, and no spill file.  The sort entry point is held to std::stable_sort on the way.
//     sorted_close_check <index prefix> <reads_1.fq> <reads_2.fq> <genome.fai> <batch pairs> <trim_qual> <scratch directory>
// Exit code 0 and "ok" when nothing differs (and the sanitizers found nothing).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <numeric>
#include <string>
#include <vector>
#include <dirent.h>
#include <unistd.h>

#include "fastquick_amd.h"

struct Fastq { std::vector<std::string> name, seq, qual; };
static Fastq read_fastq(const char *path) {
  Fastq f;
  std::ifstream in(path);
  std::string a, b, c, d;
  while (std::getline(in, a) && std::getline(in, b) && std::getline(in, c) && std::getline(in, d)) { f.name.push_back(a.substr(1, a.find_first_of(" \t") - 1)); f.seq.push_back(b); f.qual.push_back(d); }
  return f;
}
static std::string slurp(const std::string &path) {
  std::ifstream in(path, std::ios_base::binary);
  return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
#define MUST(x) do { if (x) { fprintf(stderr, "%s failed\n", #x); return 1; } } while (0)

int main(int argc, char **argv) {
  if (argc != 8) { fprintf(stderr, "usage: sorted_close_check <index prefix> <reads_1.fq> <reads_2.fq> <genome.fai> <batch pairs> <trim_qual> <scratch directory>\n"); return 2; }
  long bad = 0;
  // the sort entry point against std::stable_sort
  for (int64_t n : {0, 1, 255, 4096, 4097, 20001})
    for (int bits : {1, 9, 34, 64}) {
      std::vector<uint64_t> k((size_t)n);
      uint64_t x = 88172645463325252ull;
      for (auto &v : k) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = bits < 64 ? x & ((1ull << bits) - 1) : x; }
      std::vector<uint32_t> perm((size_t)n + 1), want((size_t)n);
      std::iota(want.begin(), want.end(), 0u);
      std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
      double ms = 0;
      MUST(fq_sort_keys_device(0, k.data(), n, bits, perm.data(), &ms));
      if (!std::equal(want.begin(), want.end(), perm.begin())) { fprintf(stderr, "fq_sort_keys_device: n = %lld, %d bits: not the stable permutation\n", (long long)n, bits); ++bad; }
    }
  Fastq fq[2] = {read_fastq(argv[2]), read_fastq(argv[3])};
  const int n = (int)fq[0].seq.size(), B = atoi(argv[5]);
  if (!n || fq[1].seq.size() != (size_t)n) { fprintf(stderr, "no reads\n"); return 2; }
  const std::string dir = argv[7];
  fq_index_t *ix = nullptr;
  MUST(fq_index_load(argv[1], 0, &ix));
  fq_opts_t o;
  fq_default_opts(&o);
  o.trim_qual = atoi(argv[6]);
  fq_qc_opts_t qo;
  fq_qc_default_opts(&qo);
  fq_ctx_t *cx = nullptr;
  MUST(fq_ctx_create(ix, &o, B, &cx));
  const char *rg = "@RG\tID:grp\tSM:s";
  const std::string path[4] = {dir + "/attached.bam", dir + "/spilled.bam", dir + "/mixed.bam", dir + "/empty.bam"};
  fq_bam_t *w[4];
  fq_bam_sort_stats_t st[4];
  MUST(fq_bam_create_sorted(ix, argv[4], path[0].c_str(), rg, &qo, (int64_t)1 << 30, &w[0]));
  MUST(fq_bam_create_sorted(ix, argv[4], path[1].c_str(), rg, &qo, 1, &w[1]));
  MUST(fq_bam_create_sorted(ix, argv[4], path[2].c_str(), rg, &qo, 1, &w[2]));      // (its limit is raised and lowered below)
  MUST(fq_bam_create_sorted(ix, argv[4], path[3].c_str(), rg, &qo, 0, &w[3]));
  for (int k = 0; k < 4; ++k) MUST(fq_bam_sort_stats_at_close(w[k], &st[k]));
  MUST(fq_ctx_attach_bam(cx, w[0]));
  long bytes = 0;
  int batches = 0;
  for (int b0 = 0; b0 < n; b0 += B, ++batches) {
    const int m = std::min(B, n - b0);
    size_t stride = 1, ns = 1;
    for (int e = 0; e < 2; ++e) for (int i = 0; i < m; ++i) { stride = std::max(stride, fq[e].seq[b0 + i].size()); ns = std::max(ns, fq[0].name[b0 + i].size() + 1); }
    std::vector<uint8_t> seq(2 * (size_t)m * stride, 0), qual(2 * (size_t)m * stride, 0);
    std::vector<int32_t> len(2 * (size_t)m);
    std::vector<char> names((size_t)m * ns, 0);
    for (int e = 0; e < 2; ++e)
      for (int i = 0; i < m; ++i) {
        const std::string &s = fq[e].seq[b0 + i], &q = fq[e].qual[b0 + i];
        memcpy(seq.data() + ((size_t)e * m + i) * stride, s.data(), s.size());
        memcpy(qual.data() + ((size_t)e * m + i) * stride, q.data(), q.size());
        len[(size_t)e * m + i] = (int32_t)s.size();
        if (!e) memcpy(names.data() + (size_t)i * ns, fq[0].name[b0 + i].data(), fq[0].name[b0 + i].size());
      }
    fq_read_batch_t rb{m, (int32_t)stride, seq.data(), qual.data(), len.data(), names.data(), (int32_t)ns, nullptr};
    fq_result_batch_t res;
    MUST(fq_align_batch(cx, &rb, &res));
    MUST(fq_bam_add_last(w[0], cx));
    const void *rec = nullptr; int64_t rec_len = 0;
    MUST(fq_bam_format_last(w[0], cx, &rec, &rec_len));
    std::vector<uint8_t> exact((const uint8_t *)rec, (const uint8_t *)rec + rec_len);      // (a heap block of exactly the run's size)
    MUST(fq_bam_write_records(w[1], exact.data(), rec_len));
    // the third writer in pieces: the first half of the records as one run, the rest as another
    int64_t cut = 0;
    while (cut < rec_len / 2) { uint32_t bs; memcpy(&bs, exact.data() + cut, 4); cut += (int64_t)bs + 4; }
    std::vector<uint8_t> head(exact.begin(), exact.begin() + cut), tail(exact.begin() + cut, exact.end());
    MUST(fq_bam_write_records(w[2], head.data(), (int64_t)head.size()));
    MUST(fq_bam_write_records(w[2], tail.empty() ? nullptr : tail.data(), (int64_t)tail.size()));
    if (rec_len > 4 && fq_bam_write_records(w[2], exact.data(), rec_len - 3) == 0) { fprintf(stderr, "a run that ends inside a record was taken\n"); ++bad; }
    std::vector<fq_bam_sort_ent_t> ent((size_t)(2 * m) + 1);
    const int64_t ne = fq_bam_sort_run_entries(w[0], -1, ent.data(), (int64_t)ent.size());
    for (int64_t i = 1; i < ne; ++i) if (ent[(size_t)i].key < ent[(size_t)i - 1].key) { fprintf(stderr, "batch at %d: the attached run is not in key order\n", b0); ++bad; break; }
    bytes += (long)rec_len;
  }
  for (int k = 0; k < 4; ++k) MUST(fq_bam_close(w[k]));
  fq_ctx_destroy(cx);
  fq_index_destroy(ix);
  const std::string f0 = slurp(path[0]), i0 = slurp(path[0] + ".bai");
  for (int k = 1; k < 3; ++k) {
    if (slurp(path[k]) != f0) { fprintf(stderr, "%s differs from %s\n", path[k].c_str(), path[0].c_str()); ++bad; }
    if (slurp(path[k] + ".bai") != i0) { fprintf(stderr, "%s.bai differs from %s.bai\n", path[k].c_str(), path[0].c_str()); ++bad; }
  }
  if (st[0].runs != batches || st[0].device_sorted_runs != batches || st[0].spilled_runs != 0 || st[1].spilled_runs != st[1].runs || st[1].device_sorted_runs != 0 || st[2].runs != 2 * batches ||
      st[0].records != st[1].records || st[0].records != st[2].records || st[3].records != 0 || st[3].runs != 0) { fprintf(stderr, "the writers' statistics do not say what they were fed\n"); ++bad; }
  if (DIR *d = opendir(dir.c_str())) {
    while (dirent *e = readdir(d)) if (strstr(e->d_name, ".tmp.")) { fprintf(stderr, "left behind: %s\n", e->d_name); ++bad; }
    closedir(d);
  }
  for (int k = 0; k < 4; ++k) { unlink(path[k].c_str()); unlink((path[k] + ".bai").c_str()); }
  if (bad || !bytes || f0.size() < 100 || i0.size() < 16) { fprintf(stderr, "%ld differences (%ld bytes of BAM records)\n", bad, bytes); return 1; }
  printf("ok: %d pairs in %d batches, %lld records, %ld bytes of records, a file of %zu bytes and an index of %zu\n", n, batches, (long long)st[0].records, bytes, f0.size(), i0.size());
  return 0;
}
