// TEST INFRASTRUCTURE ONLY: the chunked panel reader of `svd` as host loops (fq_vcf.cpp, the bodies of fq_vcf.h) under AddressSanitizer / UBSan, as a program
// of its own.  tests/test_svd_reader.py builds and runs it:
//     make && ./vcf_check <tmp dir> <panel.vcf>...
// 1. Each panel goes through the serial reader and through reader 2 at 4096-byte chunks: the panels are compared ("0 differ").
// 2. The first panel's text cut short -- mid-cell, mid-number, mid-line, at every length of its last records -- and texts of only tabs, with a cell of 70,000
//    characters and with NUL bytes: each sits at the very end of an exactly sized allocation, and the bodies (line ends by hand, fq_vcf_site_line,
//    fq_vcf_compact_line, fq_vcf_geno_line) run over it; a read outside [text, text + n) is a sanitizer report.
// 3. The same texts as files through both readers: the verdicts (panel, or message) are compared ("0 differ").
// The device entry points fq_vcf.cpp and fq_svd.cpp refer to are stubs here: reader 2 never calls them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastquick_amd.h"
#include "fq_backend.h"
#include "fq_svd.h"
#include "fq_vcf.h"

namespace fqdev {
State *state_create(int) { return nullptr; }
void state_destroy(State *) {}
int bind(State *) { return -3; }
const char *last_error() { return "no device in this build"; }
SvdDev *svd_upload(const int8_t *, int32_t, int32_t, int64_t, int64_t, const double *) { return nullptr; }
void svd_free(SvdDev *) {}
int svd_gram(SvdDev *, int32_t *) { return -3; }
int svd_apply(SvdDev *, const double *, int32_t, double *) { return -3; }
int svd_project(SvdDev *, const double *, double *) { return -3; }
void *dmalloc(size_t) { return nullptr; }
void dfree(void *) {}
int h2d(void *, const void *, size_t) { return -3; }
int d2h(void *, const void *, size_t) { return -3; }
int d2d(void *, const void *, size_t) { return -3; }
int dzero(void *, size_t) { return -3; }
int dfill(void *, int, size_t) { return -3; }
int sync() { return -3; }
const FqzCrcConst *crc_const() { return nullptr; }
int launch_inflate(const FqInflateArgs &) { return -3; }
int launch_nl_index(const uint8_t *, uint32_t, uint32_t, uint32_t *, uint32_t, uint32_t *) { return -3; }
int launch_scan(const uint32_t *, uint64_t *, uint32_t) { return -3; }
int launch_vcf_site(const FqVcfSiteArgs &) { return -3; }
int launch_vcf_compact(const uint32_t *, const uint64_t *, uint32_t *, uint32_t) { return -3; }
int launch_vcf_geno(const FqVcfGenoArgs &) { return -3; }
}  // namespace fqdev
extern "C" int fq_host_cpus(void) { return 2; }

struct Verdict { int rc = 0; std::string msg; std::vector<int8_t> g; std::vector<int32_t> pos; std::vector<std::string> chrom, samples; };
static Verdict read_with(int reader, const std::string &path) {
  Verdict v;
  fq_svd_opts_t o;
  fq_svd_default_opts(&o);
  o.host_eval = 1; o.host_threads = 2; o.reader = reader; o.chunk_bytes = 4096;
  fq_svd_t *p = nullptr;
  if (fq_svd_create(&o, &p)) { v.rc = -99; return v; }
  const char *paths[1] = {path.c_str()};
  v.rc = reader ? fq_svd_read_panel(p, paths, 1, nullptr) : fq_svd_read_vcf(p, path.c_str());
  if (v.rc) v.msg = fq_svd_last_error(p);
  else {
    fq_svd_result_t r;
    fq_svd_result(p, &r);
    v.g.resize((size_t)r.n_marker * r.n_sample); v.pos.resize(r.n_marker);
    std::vector<const char *> c(r.n_marker), s(r.n_sample);
    fq_svd_panel(p, v.g.data(), v.pos.data(), c.data(), s.data());
    for (auto x : c) v.chrom.push_back(x);
    for (auto x : s) v.samples.push_back(x);
  }
  fq_svd_destroy(p);
  return v;
}
static int differ(const std::string &path) {
  const Verdict a = read_with(0, path), b = read_with(2, path);
  const bool same = a.rc == b.rc && a.msg == b.msg && a.g == b.g && a.pos == b.pos && a.chrom == b.chrom && a.samples == b.samples;
  if (!same) fprintf(stderr, "vcf_check: %s: serial (%d) '%s', %zu genotypes; chunked (%d) '%s', %zu genotypes\n", path.c_str(), a.rc, a.msg.c_str(), a.g.size(), b.rc, b.msg.c_str(), b.g.size());
  return same ? 0 : 1;
}

// the bodies over text[0, n), which ends with the allocation
static void bodies(const std::string &text, int n_sample) {
  const uint32_t n = (uint32_t)text.size();
  uint8_t *T = (uint8_t *)malloc(n ? n : 1);
  memcpy(T, text.data(), n);
  std::vector<uint32_t> nl;
  for (uint32_t i = 0; i < n; ++i) if (T[i] == '\n') nl.push_back(i);
  if (n && T[n - 1] != '\n') nl.push_back(n);      // (the reader gives a last line its line end; here the line simply ends with the text)
  const uint32_t L = (uint32_t)nl.size();
  std::vector<FqVcfLine> line(L);
  std::vector<uint32_t> keep(L), kept(L);
  std::vector<uint64_t> off(L + 1);
  FqVcfSiteArgs a{};
  a.text = T; a.n = n; a.lo = 0; a.nl = nl.data(); a.n_lines = L; a.line = line.data(); a.keep = keep.data();
  for (uint32_t i = 0; i < L; ++i) fq_vcf_site_line(a, i);
  uint64_t run = 0;
  for (uint32_t i = 0; i < L; ++i) { off[i] = run; run += keep[i]; }
  for (uint32_t i = 0; i < L; ++i) fq_vcf_compact_line(keep.data(), off.data(), kept.data(), i);
  std::vector<int8_t> g((size_t)run * n_sample + 1);
  std::vector<uint32_t> needs((size_t)run + 1);
  FqVcfGenoArgs ga{};
  ga.text = T; ga.n = n; ga.line = line.data(); ga.kept = kept.data(); ga.n_kept = (uint32_t)run; ga.n_sample = n_sample; ga.g = g.data(); ga.needs_host = needs.data();
  for (uint32_t k = 0; k < (uint32_t)run; ++k) fq_vcf_geno_line(ga, k);
  free(T);
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: vcf_check TMP_DIR PANEL.vcf...\n"); return 2; }
  int total = 0;
  for (int k = 2; k < argc; ++k) { const int d = differ(argv[k]); total += d; printf("vcf_check: %s, %d differ\n", argv[k], d); }
  std::string text;
  {
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
  }
  const size_t hdr = text.find('\n', text.find("#CHROM")) + 1;
  int n_sample = 0;
  for (size_t i = text.find("#CHROM"); i < hdr; ++i) n_sample += text[i] == '\t';
  n_sample -= 8;
  std::vector<std::string> cases;
  for (size_t cut = text.size(); cut + 400 > text.size() && cut > hdr; --cut) cases.push_back(text.substr(0, cut));      // mid-line, mid-cell, mid-number: every length
  const std::string body = text.substr(hdr), head = text.substr(0, hdr);
  cases.push_back(head + body + std::string(300, '\t') + "\n" + body);                                  // a line of only tabs
  cases.push_back(head + body + "1\t77\t.\tA\tC\t.\t.\t.\tGT\t" + std::string(70000, '1') + "\t0/1\n");      // a cell of 70,000 characters
  cases.push_back(head + body + "1\t78\t.\tA\tC\t.\t.\t.\tGT\t0/1\t0" + std::string(1, '\0') + "1\t1/1\n");     // NUL bytes in a cell
  cases.push_back(head + body + "2" + std::string(1, '\0') + "2\t79\t.\tA\tC\t.\t.\t.\tGT\t0/1\n");              // ... and in CHROM
  cases.push_back(head + body + "1\t80\t.\tA\tC\t.\t.\t.\tGT:PL\t0/1:1,2\t0/1:1,2,\t0/1:,1,2,3");        // a PL that ends early, at the text's end
  int cut_differ = 0;
  const std::string tmp = std::string(argv[1]) + "/cut.vcf";
  for (size_t c = 0; c < cases.size(); ++c) {
    bodies(cases[c], n_sample);
    bodies(cases[c].substr(hdr), n_sample);      // (the records alone: the first line begins at the allocation's first byte)
    if (c % 16 == 0 || c + 8 > cases.size()) {   // (through the files: every sixteenth cut, and the made-up lines)
      FILE *f = fopen(tmp.c_str(), "wb");
      if (!f) return 2;
      fwrite(cases[c].data(), 1, cases[c].size(), f);
      fclose(f);
      cut_differ += differ(tmp);
    }
  }
  remove(tmp.c_str());
  printf("vcf_check: %zu cut and made-up texts, %d differ\n", cases.size(), cut_differ);
  return total + cut_differ ? 1 : 0;
}
