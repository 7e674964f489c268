// fq_svd_host.h -- what the two VCF readers of `svd` share on the host: the fq_svd object, libVcf's tokenising, and SVDcalculator::ReadVcf's statement for ONE
// record (fq_svd_record).  The serial reader (fq_svd.cpp: read_vcf) runs it over every line; the chunked reader (fq_vcf.cpp) over the lines its kernels
// hand back (needs_host).  Both install a kept marker through fq_svd_install, so the error texts, the `(line N of path)` and the panel are the same.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "fastquick_amd.h"
#include "fq_svd.h"

struct fq_svd {
  fq_svd_opts_t o{};
  std::string err;
  // the panel: genotypes markers x samples as ReadVcf keeps them, the kept markers' sites, chooseBed
  int32_t M = 0, N = 0;
  std::vector<int8_t> g;
  std::vector<std::string> samples, chrom;
  std::vector<int32_t> pos;
  std::unordered_map<std::string, std::unordered_map<int32_t, std::pair<char, char>>> bed;
  // the decomposition
  std::vector<double> mu, ud, v, sigma;
  int32_t iterations = 0;
  double residual = 0, lambda0 = 0;
  double t_read = 0, t_gram = 0, t_iter = 0, t_project = 0, t_write = 0;
  bool ran = false;
  // the sample-major padded matrix of fq_svd.h, and the device
  int32_t n_pad = 0;
  int64_t m_pad = 0;
  std::vector<int8_t> gt;
  std::vector<double> c;      // host_eval: the centred Gram matrix
  fqdev::State *dev = nullptr;
  fqdev::SvdDev *dd = nullptr;
  fq_svd_read_stats_t rs{};   // the chunked reader's counts and seconds (fq_svd_read_stats)

  int fail(int rc, const std::string &m) { err = m; return rc; }
};

namespace fqsvd {

// String::AsInteger: an optional '-', an optional 0x, digits up to the first character that is none
inline long as_integer(const char *s, size_t len) {
  long v = 0;
  int base = 10;
  size_t i = 0;
  long sign = 1;
  if (i == len) return 0;
  if (s[i] == '-') { sign = -1; ++i; }
  if (len > i + 2 && s[i] == '0' && (s[i + 1] == 'x' || s[i + 1] == 'X')) { base = 16; i += 2; }
  for (; i < len; ++i) {
    const int d = s[i] >= 'a' && s[i] <= 'z' ? s[i] - 32 : s[i];
    if (d >= '0' && d <= '9') v = (long)((unsigned long)v * base + (unsigned long)(d - '0'));
    else if (d >= 'A' && d <= 'F' && base == 16) v = (long)((unsigned long)v * base + (unsigned long)(d - 'A' + 10));
    else break;
  }
  return sign * v;
}
struct Span { const char *p; size_t n; };
// StringArray::ReplaceColumns: every separator ends a column, empty ones included
inline void columns(const char *p, size_t n, char sep, std::vector<Span> &out) {
  out.clear();
  size_t a = 0;
  for (size_t i = 0; i <= n; ++i)
    if (i == n || p[i] == sep) { out.push_back({p + a, i - a}); a = i + 1; }
}
// StringArray::ReplaceTokens: runs of separators are skipped, no empty token
inline void tokens(const char *p, size_t n, const char *seps, std::vector<Span> &out) {
  out.clear();
  size_t i = 0;
  while (i < n) {
    while (i < n && strchr(seps, p[i])) ++i;
    const size_t a = i;
    while (i < n && !strchr(seps, p[i])) ++i;
    if (a < n) out.push_back({p + a, i - a});
  }
}
inline bool is(const Span &s, const char *lit) { return s.n == strlen(lit) && !memcmp(s.p, lit, s.n); }
inline int find_key(const std::vector<Span> &keys, const char *k) {
  for (size_t i = 0; i < keys.size(); ++i) if (is(keys[i], k)) return (int)i;
  return -1;
}
inline bool accept_chrom(const std::string &c) {   // acceptChr: 1 .. 22, chr1 .. chr22
  const char *s = c.c_str();
  if (!strncmp(s, "chr", 3)) s += 3;
  const size_t n = strlen(s);
  if (n < 1 || n > 2 || s[0] < '1' || s[0] > '9' || (n == 2 && (s[1] < '0' || s[1] > '9'))) return false;
  const int v = atoi(s);
  return v >= 1 && v <= 22;
}

// what a reader carries from record to record
struct RecState {
  std::string path;            // (of the file the line numbers count in)
  int64_t line_no = 0;
  std::string prev_chrom;      // the previously kept marker ("Duplicated Marker"): across the files of a list
  int32_t prev_pos = 0;
  bool have_prev = false;
  std::vector<Span> tok, keys, cell, val;
  std::vector<int8_t> row;
  std::string where() const { return " (line " + std::to_string(line_no) + " of " + path + ")"; }
};
enum { FQ_REC_KEPT = 0, FQ_REC_SKIPPED = 1 };   // (negative: refused, p->err says why)

// a kept marker into the object
inline int fq_svd_install(fq_svd *p, RecState &S, const std::string &chrom, int32_t pos, char ref, char alt, const int8_t *row) {
  if (p->M == FQ_SVD_MAX_MARKERS) return p->fail(FQ_ELIMIT, "svd: more than 2^29 markers");
  p->bed[chrom][pos] = std::make_pair((char)toupper((unsigned char)ref), (char)toupper((unsigned char)alt));
  p->chrom.push_back(chrom);
  p->pos.push_back(pos);
  p->g.insert(p->g.end(), row, row + p->N);
  p->M++;
  S.prev_chrom = chrom; S.prev_pos = pos; S.have_prev = true;
  return FQ_REC_KEPT;
}

// SVDcalculator::ReadVcf's body for the record ln[0, n) (no line end, not empty)
inline int fq_svd_record(fq_svd *p, RecState &S, const char *ln, size_t n) {
  const int maxPhred = 255;
  std::vector<Span> &tok = S.tok, &keys = S.keys, &cell = S.cell, &val = S.val;
  S.row.assign(p->N, -1);
  columns(ln, n, '\t', tok);
  if (tok.size() < 5) return p->fail(FQ_EINVAL, "a record with fewer than five columns" + S.where());
  const std::string chrom(tok[0].p, tok[0].n);
  const int32_t pos = atoi(std::string(tok[1].p, tok[1].n).c_str());
  // (the names chrom:pos of this record and of the previously kept marker are equal exactly when both parts are: a kept marker's chromosome has no ':')
  if (S.have_prev && S.prev_pos == pos && S.prev_chrom == chrom) return p->fail(FQ_EINVAL, "Duplicated Marker at " + chrom + ":" + std::to_string(pos) + S.where());
  if (!accept_chrom(chrom)) return FQ_REC_SKIPPED;
  size_t alt_len = 0;
  while (alt_len < tok[4].n && tok[4].p[alt_len] != ',') ++alt_len;   // of several ALT alleles the first
  if (tok[3].n > 1 || alt_len > 1) return FQ_REC_SKIPPED;
  if (tok[3].n == 0 || alt_len == 0) return p->fail(FQ_EINVAL, "an empty REF or ALT allele" + S.where());
  if (tok.size() < 10) return p->fail(FQ_EINVAL, "a record without FORMAT and genotype columns" + S.where());
  columns(tok[8].p, tok[8].n, ':', keys);
  int idx = find_key(keys, "PL"), flag = 0;   // 0 for PL, 1 for GL, 2 for GT
  if (idx < 0) {
    idx = find_key(keys, "GL");
    if (idx >= 0) flag = 1;
    else {
      idx = find_key(keys, "GT");
      if (idx >= 0) flag = 2;
      else return p->fail(FQ_EINVAL, "Cannot recognize GT, GL or PL key in FORMAT field" + S.where());
    }
  }
  const size_t first = (tok[9].n == 0 && tok.size() > 10) ? 10 : 9;   // (libVcf steps over an empty column behind FORMAT)
  if (tok.size() - first != (size_t)p->N) return p->fail(FQ_EINVAL, "a record with " + std::to_string(tok.size() - first) + " genotype columns under " + std::to_string(p->N) + " sample names" + S.where());
  for (int32_t i = 0; i < p->N; ++i) {
    const Span &sv = tok[first + i];
    Span value;
    if (is(sv, "./.") || is(sv, ".")) value = idx == 0 ? Span{"./.", 3} : Span{"", 0};   // (libVcf: the first value "./.", the others empty)
    else {
      columns(sv.p, sv.n, ':', cell);
      if (cell.size() != keys.size()) return p->fail(FQ_EINVAL, "# values = " + std::string(sv.p, sv.n) + " do not match with # fields in FORMAT field = " + std::to_string(keys.size()) + " at sampleIndex = " + std::to_string(i) + S.where());
      value = cell[idx];
    }
    long phred11, phred12, phred22;
    if (flag == 2) {
      tokens(value.p, value.n, "|/", val);
      if (val.size() < 2) return p->fail(FQ_EINVAL, "a GT with fewer than two alleles: '" + std::string(value.p, value.n) + "', sample " + std::to_string(i) + S.where());
      const long geno = as_integer(val[0].p, val[0].n) + as_integer(val[1].p, val[1].n);
      if (geno == 0) { phred11 = 0; phred12 = 30; phred22 = 50; }
      else if (geno == 1) { phred11 = 50; phred12 = 0; phred22 = 50; }
      else { phred11 = 50; phred12 = 30; phred22 = 0; }
    } else {
      tokens(value.p, value.n, ",", val);
      if (val.size() < 3) return p->fail(FQ_EINVAL, std::string("a ") + (flag ? "GL" : "PL") + " with fewer than three values: '" + std::string(value.p, value.n) + "', sample " + std::to_string(i) + S.where());
      long ph[3];
      for (int k = 0; k < 3; ++k) {
        if (flag == 0) ph[k] = as_integer(val[k].p, val[k].n);
        else {
          const double x = -10. * atof(std::string(val[k].p, val[k].n).c_str());
          if (!(x > -2147483648. && x < 2147483648.)) return p->fail(FQ_EINVAL, "a GL beyond what an int holds" + S.where());
          ph[k] = static_cast<int>(x);
        }
      }
      phred11 = ph[0]; phred12 = ph[1]; phred22 = ph[2];
    }
    if (phred11 < 0 || phred12 < 0 || phred22 < 0) return p->fail(FQ_EINVAL, "Negative PL or Positive GL observed" + S.where());
    if (phred11 > maxPhred) phred11 = maxPhred;
    if (phred12 > maxPhred) phred12 = maxPhred;
    if (phred22 > maxPhred) phred22 = maxPhred;
    int minGeno = -1;
    long minPhred = maxPhred;
    if (phred11 < minPhred) { minPhred = phred11; minGeno = 0; }
    if (phred12 < minPhred) { minPhred = phred12; minGeno = 1; }
    if (phred22 < minPhred) { minPhred = phred22; minGeno = 2; }
    S.row[i] = (int8_t)minGeno;
  }
  return fq_svd_install(p, S, chrom, pos, tok[3].p[0], tok[4].p[0], S.row.data());
}

// the header line #CHROM ...: the sample names behind FORMAT
inline void header_samples(const char *ln, size_t n, std::vector<std::string> &out) {
  std::vector<Span> tok;
  columns(ln, n, '\t', tok);
  out.clear();
  for (size_t i = 9; i < tok.size(); ++i) out.emplace_back(tok[i].p, tok[i].n);
}

}  // namespace fqsvd
