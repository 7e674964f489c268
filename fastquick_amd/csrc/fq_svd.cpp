// fq_svd.cpp -- `FASTQuick pop+con --RefVCF` (VerifyBamID2's SVDcalculator) around the statements of fq_svd.h: the subcommand `svd`.
//
// Host side: the VCF reader (SVDcalculator::ReadVcf, SVDcalculator.cpp:18-193, with libVcf's tokenising of a record: libVcfFile.cpp:473-530, :910-940,
// and String::AsInteger, StringBasics.cpp:1015-1068), the block subspace iteration with its orthonormalisation and Rayleigh-Ritz step, the sign rule
// and the writers (WriteSVD, SVDcalculator.cpp:248-279).  The five statements of fq_svd.h run in its kernels (fq_device.hip: svd_gram, svd_apply,
// svd_project) or -- opts.host_eval -- as host loops over the same int8 matrix: the CPU tier.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include <zlib.h>

#include "fastquick_amd.h"
#include "fq_backend.h"
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

  int fail(int rc, const std::string &m) { err = m; return rc; }
};

namespace {

thread_local std::string g_create_err;

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int n_threads(const fq_svd *p) {
  const int nt = p->o.host_threads > 0 ? p->o.host_threads : std::min(16, fq_host_cpus());
  return std::max(1, std::min(nt, 16));
}
// fn(a, b) over [0, n) in contiguous ranges, one a thread
void parallel_for(int64_t n, int nt, const std::function<void(int64_t, int64_t)> &fn) {
  if (nt <= 1 || n < 2 * nt) { fn(0, n); return; }
  std::vector<std::thread> th;
  const int64_t step = (n + nt - 1) / nt;
  for (int64_t a = 0; a < n; a += step) th.emplace_back(fn, a, std::min(n, a + step));
  for (auto &t : th) t.join();
}

// String::AsInteger: an optional '-', an optional 0x, digits up to the first character that is none
long as_integer(const char *s, size_t len) {
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
void columns(const char *p, size_t n, char sep, std::vector<Span> &out) {
  out.clear();
  size_t a = 0;
  for (size_t i = 0; i <= n; ++i)
    if (i == n || p[i] == sep) { out.push_back({p + a, i - a}); a = i + 1; }
}
// StringArray::ReplaceTokens: runs of separators are skipped, no empty token
void tokens(const char *p, size_t n, const char *seps, std::vector<Span> &out) {
  out.clear();
  size_t i = 0;
  while (i < n) {
    while (i < n && strchr(seps, p[i])) ++i;
    const size_t a = i;
    while (i < n && !strchr(seps, p[i])) ++i;
    if (a < n) out.push_back({p + a, i - a});
  }
}
bool is(const Span &s, const char *lit) { return s.n == strlen(lit) && !memcmp(s.p, lit, s.n); }
int find_key(const std::vector<Span> &keys, const char *k) {
  for (size_t i = 0; i < keys.size(); ++i) if (is(keys[i], k)) return (int)i;
  return -1;
}
bool accept_chrom(const std::string &c) {   // acceptChr: 1 .. 22, chr1 .. chr22
  const char *s = c.c_str();
  if (!strncmp(s, "chr", 3)) s += 3;
  const size_t n = strlen(s);
  if (n < 1 || n > 2 || s[0] < '1' || s[0] > '9' || (n == 2 && (s[1] < '0' || s[1] > '9'))) return false;
  const int v = atoi(s);
  return v >= 1 && v <= 22;
}

void clear_panel(fq_svd *p) {
  if (p->dd) { if (p->dev && !fqdev::bind(p->dev)) fqdev::svd_free(p->dd); p->dd = nullptr; }
  p->M = p->N = 0;
  p->g.clear(); p->samples.clear(); p->chrom.clear(); p->pos.clear(); p->bed.clear();
  p->gt.clear(); p->c.clear();
  p->ran = false;
}

int read_text(fq_svd *p, const char *path, std::string &text) {   // plain, gzip or BGZF: zlib reads all three
  gzFile f = gzopen(path, "rb");
  if (!f) return p->fail(FQ_EIO, std::string("Failed opening file ") + path);
  gzbuffer(f, 1 << 20);
  std::vector<char> buf(1 << 22);
  for (;;) {
    const int got = gzread(f, buf.data(), (unsigned)buf.size());
    if (got < 0) { int en = 0; const std::string m = gzerror(f, &en); gzclose(f); return p->fail(FQ_EIO, std::string(path) + ": " + m); }
    if (got == 0) break;
    text.append(buf.data(), (size_t)got);
  }
  gzclose(f);
  return 0;
}

// SVDcalculator::ReadVcf
int read_vcf(fq_svd *p, const char *path) {
  std::string text;
  if (int rc = read_text(p, path, text)) return rc;
  const int maxPhred = 255;
  bool have_header = false;
  std::string prev_name, name;
  std::vector<Span> tok, keys, cell, val;
  std::vector<int8_t> row;
  size_t at = 0;
  int64_t line_no = 0;
  auto where = [&]() { return " (line " + std::to_string(line_no) + " of " + path + ")"; };
  while (at < text.size()) {
    size_t e = text.find('\n', at);
    if (e == std::string::npos) e = text.size();
    const char *ln = text.data() + at;
    size_t n = e - at;
    at = e + 1;
    ++line_no;
    if (n && ln[n - 1] == '\r') --n;
    if (!have_header) {
      if (n >= 2 && ln[0] == '#' && ln[1] == '#') continue;
      if (n >= 2 && ln[0] == '#' && ln[1] == 'C') {
        columns(ln, n, '\t', tok);
        for (size_t i = 9; i < tok.size(); ++i) p->samples.emplace_back(tok[i].p, tok[i].n);
        have_header = true;
        if (p->samples.empty()) return p->fail(FQ_EINVAL, std::string("No individual genotype information exist in the input VCF file ") + path);
        p->N = (int32_t)p->samples.size();
        row.assign(p->N, -1);
        continue;
      }
      return p->fail(FQ_EINVAL, "Header line is not found : #CHROM..." + where());
    }
    if (n == 0) break;   // (the reference's reader ends at an empty line)
    columns(ln, n, '\t', tok);
    if (tok.size() < 5) return p->fail(FQ_EINVAL, "a record with fewer than five columns" + where());
    const std::string chrom(tok[0].p, tok[0].n);
    const int32_t pos = atoi(std::string(tok[1].p, tok[1].n).c_str());
    name = chrom + ":" + std::to_string(pos);
    if (prev_name == name) return p->fail(FQ_EINVAL, "Duplicated Marker at " + name + where());
    if (!accept_chrom(chrom)) continue;
    size_t alt_len = 0;
    while (alt_len < tok[4].n && tok[4].p[alt_len] != ',') ++alt_len;   // of several ALT alleles the first
    if (tok[3].n > 1 || alt_len > 1) continue;
    if (tok[3].n == 0 || alt_len == 0) return p->fail(FQ_EINVAL, "an empty REF or ALT allele" + where());
    if (tok.size() < 10) return p->fail(FQ_EINVAL, "a record without FORMAT and genotype columns" + where());
    const char ref = (char)toupper((unsigned char)tok[3].p[0]), alt = (char)toupper((unsigned char)tok[4].p[0]);
    columns(tok[8].p, tok[8].n, ':', keys);
    int idx = find_key(keys, "PL"), flag = 0;   // 0 for PL, 1 for GL, 2 for GT
    if (idx < 0) {
      idx = find_key(keys, "GL");
      if (idx >= 0) flag = 1;
      else {
        idx = find_key(keys, "GT");
        if (idx >= 0) flag = 2;
        else return p->fail(FQ_EINVAL, "Cannot recognize GT, GL or PL key in FORMAT field" + where());
      }
    }
    const size_t first = (tok[9].n == 0 && tok.size() > 10) ? 10 : 9;   // (libVcf steps over an empty column behind FORMAT)
    if (tok.size() - first != (size_t)p->N) return p->fail(FQ_EINVAL, "a record with " + std::to_string(tok.size() - first) + " genotype columns under " + std::to_string(p->N) + " sample names" + where());
    for (int32_t i = 0; i < p->N; ++i) {
      const Span &sv = tok[first + i];
      Span value;
      if (is(sv, "./.") || is(sv, ".")) value = idx == 0 ? Span{"./.", 3} : Span{"", 0};   // (libVcf: the first value "./.", the others empty)
      else {
        columns(sv.p, sv.n, ':', cell);
        if (cell.size() != keys.size()) return p->fail(FQ_EINVAL, "# values = " + std::string(sv.p, sv.n) + " do not match with # fields in FORMAT field = " + std::to_string(keys.size()) + " at sampleIndex = " + std::to_string(i) + where());
        value = cell[idx];
      }
      long phred11, phred12, phred22;
      if (flag == 2) {
        tokens(value.p, value.n, "|/", val);
        if (val.size() < 2) return p->fail(FQ_EINVAL, "a GT with fewer than two alleles: '" + std::string(value.p, value.n) + "', sample " + std::to_string(i) + where());
        const long geno = as_integer(val[0].p, val[0].n) + as_integer(val[1].p, val[1].n);
        if (geno == 0) { phred11 = 0; phred12 = 30; phred22 = 50; }
        else if (geno == 1) { phred11 = 50; phred12 = 0; phred22 = 50; }
        else { phred11 = 50; phred12 = 30; phred22 = 0; }
      } else {
        tokens(value.p, value.n, ",", val);
        if (val.size() < 3) return p->fail(FQ_EINVAL, std::string("a ") + (flag ? "GL" : "PL") + " with fewer than three values: '" + std::string(value.p, value.n) + "', sample " + std::to_string(i) + where());
        long ph[3];
        for (int k = 0; k < 3; ++k) {
          if (flag == 0) ph[k] = as_integer(val[k].p, val[k].n);
          else {
            const double x = -10. * atof(std::string(val[k].p, val[k].n).c_str());
            if (!(x > -2147483648. && x < 2147483648.)) return p->fail(FQ_EINVAL, "a GL beyond what an int holds" + where());
            ph[k] = static_cast<int>(x);
          }
        }
        phred11 = ph[0]; phred12 = ph[1]; phred22 = ph[2];
      }
      if (phred11 < 0 || phred12 < 0 || phred22 < 0) return p->fail(FQ_EINVAL, "Negative PL or Positive GL observed" + where());
      if (phred11 > maxPhred) phred11 = maxPhred;
      if (phred12 > maxPhred) phred12 = maxPhred;
      if (phred22 > maxPhred) phred22 = maxPhred;
      int minGeno = -1;
      long minPhred = maxPhred;
      if (phred11 < minPhred) { minPhred = phred11; minGeno = 0; }
      if (phred12 < minPhred) { minPhred = phred12; minGeno = 1; }
      if (phred22 < minPhred) { minPhred = phred22; minGeno = 2; }
      row[i] = (int8_t)minGeno;
    }
    if (p->M == FQ_SVD_MAX_MARKERS) return p->fail(FQ_ELIMIT, "svd: more than 2^29 markers");
    p->bed[chrom][pos] = std::make_pair(ref, alt);
    p->chrom.push_back(chrom);
    p->pos.push_back(pos);
    p->g.insert(p->g.end(), row.begin(), row.end());
    p->M++;
    prev_name = name;
  }
  if (!have_header) return p->fail(FQ_EINVAL, std::string("Header line is not found : #CHROM... (") + path + ")");
  return 0;
}

// the padded sample-major matrix and the means
void make_gt(fq_svd *p) {
  if (!p->gt.empty()) return;
  p->n_pad = (p->N + FQ_SVD_TILE - 1) / FQ_SVD_TILE * FQ_SVD_TILE;
  p->m_pad = ((int64_t)p->M + FQ_SVD_TILE - 1) / FQ_SVD_TILE * FQ_SVD_TILE;
  p->gt.assign((size_t)p->n_pad * p->m_pad, 0);
  p->mu.assign(p->M, 0.);
  parallel_for(p->M, n_threads(p), [&](int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      const int8_t *r = p->g.data() + (size_t)i * p->N;
      int32_t s = 0;
      for (int32_t j = 0; j < p->N; ++j) { s += r[j]; p->gt[(size_t)j * p->m_pad + i] = r[j]; }
      p->mu[i] = fq_svd_mean(s, p->N);
    }
  });
}

int open_device(fq_svd *p) {
  if (!p->dev) {
    p->dev = fqdev::state_create(p->o.device);
    if (!p->dev) return p->fail(FQ_ENODEV, std::string("svd: no device for the kernels (") + fqdev::last_error() + "); --host_eval runs the host loops");
  }
  if (fqdev::bind(p->dev)) return p->fail(FQ_ENODEV, fqdev::last_error());
  if (!p->dd) {
    p->dd = fqdev::svd_upload(p->gt.data(), p->N, p->n_pad, p->M, p->m_pad, p->mu.data());
    if (!p->dd) return p->fail(FQ_ENODEV, std::string("svd: ") + fqdev::last_error());
  }
  return 0;
}

// statements 1 to 3 on the host: A (tiles on or above the diagonal, mirrored), t and q, C
void host_gram(fq_svd *p, int32_t *a_out, bool centre) {
  const int32_t N = p->N;
  const int64_t M = p->M;
  std::vector<int32_t> A((size_t)N * N);
  parallel_for(N, n_threads(p), [&](int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j)
      for (int32_t k = (int32_t)j; k < N; ++k) A[(size_t)j * N + k] = fq_svd_dot(p->gt.data() + (size_t)j * p->m_pad, p->gt.data() + (size_t)k * p->m_pad, M);
  });
  for (int32_t j = 0; j < N; ++j) for (int32_t k = 0; k < j; ++k) A[(size_t)j * N + k] = A[(size_t)k * N + j];
  if (a_out) memcpy(a_out, A.data(), A.size() * 4);
  if (!centre) return;
  std::vector<double> tq((size_t)N + 1, 0.);
  parallel_for(N, n_threads(p), [&](int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; ++j) {
      const int8_t *g = p->gt.data() + (size_t)j * p->m_pad;
      double s = 0;
      for (int64_t i = 0; i < M; ++i) s += fq_svd_t_term(p->mu[i], g[i]);
      tq[j] = s;
    }
  });
  for (int64_t i = 0; i < M; ++i) tq[N] += p->mu[i] * p->mu[i];
  p->c.assign((size_t)N * N, 0.);
  for (int32_t j = 0; j < N; ++j) for (int32_t k = 0; k < N; ++k) p->c[(size_t)j * N + k] = fq_svd_centre(A[(size_t)j * N + k], tq[j], tq[k], tq[N]);
}

// cyclic Jacobi on the symmetric b x b matrix h (row-major, destroyed): eigenvalues descending in lam, eigenvectors the columns of w
void jacobi_eig(std::vector<double> &h, int b, std::vector<double> &lam, std::vector<double> &w) {
  w.assign((size_t)b * b, 0.);
  for (int i = 0; i < b; ++i) w[(size_t)i * b + i] = 1.;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0, diag = 0;
    for (int i = 0; i < b; ++i) { diag += h[(size_t)i * b + i] * h[(size_t)i * b + i]; for (int j = i + 1; j < b; ++j) off += h[(size_t)i * b + j] * h[(size_t)i * b + j]; }
    if (off <= 1e-60 * diag || off == 0) break;
    for (int pi = 0; pi < b - 1; ++pi)
      for (int qi = pi + 1; qi < b; ++qi) {
        const double apq = h[(size_t)pi * b + qi];
        if (apq == 0) continue;
        const double theta = (h[(size_t)qi * b + qi] - h[(size_t)pi * b + pi]) / (2 * apq);
        const double t = (theta >= 0 ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1));
        const double cs = 1 / sqrt(t * t + 1), sn = t * cs;
        for (int k = 0; k < b; ++k) {   // columns p, q
          const double hp = h[(size_t)k * b + pi], hq = h[(size_t)k * b + qi];
          h[(size_t)k * b + pi] = cs * hp - sn * hq;
          h[(size_t)k * b + qi] = sn * hp + cs * hq;
        }
        for (int k = 0; k < b; ++k) {   // rows p, q
          const double hp = h[(size_t)pi * b + k], hq = h[(size_t)qi * b + k];
          h[(size_t)pi * b + k] = cs * hp - sn * hq;
          h[(size_t)qi * b + k] = sn * hp + cs * hq;
        }
        for (int k = 0; k < b; ++k) {
          const double wp = w[(size_t)k * b + pi], wq = w[(size_t)k * b + qi];
          w[(size_t)k * b + pi] = cs * wp - sn * wq;
          w[(size_t)k * b + qi] = sn * wp + cs * wq;
        }
      }
  }
  std::vector<int> order(b);
  for (int i = 0; i < b; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return h[(size_t)x * b + x] > h[(size_t)y * b + y]; });
  lam.resize(b);
  std::vector<double> ws((size_t)b * b);
  for (int c = 0; c < b; ++c) {
    lam[c] = h[(size_t)order[c] * b + order[c]];
    for (int k = 0; k < b; ++k) ws[(size_t)k * b + c] = w[(size_t)k * b + order[c]];
  }
  w.swap(ws);
}

// modified Gram-Schmidt over the columns of z (n x b row-major), two passes a column; a column that vanishes is left zero
void orthonormalise(std::vector<double> &z, int n, int b) {
  std::vector<double> col((size_t)b * n);   // column-major while working
  for (int j = 0; j < n; ++j) for (int c = 0; c < b; ++c) col[(size_t)c * n + j] = z[(size_t)j * b + c];
  for (int c = 0; c < b; ++c) {
    double *x = col.data() + (size_t)c * n;
    double n0 = 0;
    for (int j = 0; j < n; ++j) n0 += x[j] * x[j];
    for (int pass = 0; pass < 2; ++pass)
      for (int d = 0; d < c; ++d) {
        const double *y = col.data() + (size_t)d * n;
        double dot = 0;
        for (int j = 0; j < n; ++j) dot += x[j] * y[j];
        for (int j = 0; j < n; ++j) x[j] -= dot * y[j];
      }
    double nn = 0;
    for (int j = 0; j < n; ++j) nn += x[j] * x[j];
    if (!(nn > 1e-24 * n0) || nn == 0) { for (int j = 0; j < n; ++j) x[j] = 0; continue; }   // (inside the span of the columns before it)
    const double inv = 1 / sqrt(nn);
    for (int j = 0; j < n; ++j) x[j] *= inv;
  }
  for (int j = 0; j < n; ++j) for (int c = 0; c < b; ++c) z[(size_t)j * b + c] = col[(size_t)c * n + j];
}

// statement 4 (Y = C Q) by the switch
int apply(fq_svd *p, const std::vector<double> &q, int b, std::vector<double> &y) {
  const int32_t N = p->N;
  y.resize((size_t)N * b);
  if (p->o.host_eval) {
    parallel_for(N, n_threads(p), [&](int64_t lo, int64_t hi) {
      for (int64_t j = lo; j < hi; ++j)
        for (int c = 0; c < b; ++c) y[(size_t)j * b + c] = fq_svd_apply(p->c.data() + (size_t)j * N, q.data(), N, b, c);
    });
    return 0;
  }
  if (fqdev::svd_apply(p->dd, q.data(), b, y.data())) return p->fail(FQ_ENODEV, std::string("svd: ") + fqdev::last_error());
  return 0;
}

// the leading FQ_SVD_NPC eigenpairs of C by block subspace iteration with a Rayleigh-Ritz step; stops on the residual
int iterate(fq_svd *p, std::vector<double> &lam10) {
  const int32_t N = p->N;
  const int b = std::min<int32_t>(N, FQ_SVD_BLOCK_MAX);
  std::vector<double> q((size_t)N * b), y, h((size_t)b * b), lam, w, z((size_t)N * b);
  uint32_t s = 0x9e3779b9u;   // the start block: a fixed sequence
  for (auto &x : q) { s = s * 1664525u + 1013904223u; x = (double)(s >> 8) / 8388608. - 1.; }
  orthonormalise(q, N, b);
  for (int it = 1; it <= p->o.max_iter; ++it) {
    if (int rc = apply(p, q, b, y)) return rc;
    for (int c = 0; c < b; ++c)
      for (int d = c; d < b; ++d) {
        double a1 = 0, a2 = 0;
        for (int32_t j = 0; j < N; ++j) { a1 += q[(size_t)j * b + c] * y[(size_t)j * b + d]; a2 += q[(size_t)j * b + d] * y[(size_t)j * b + c]; }
        h[(size_t)c * b + d] = h[(size_t)d * b + c] = 0.5 * (a1 + a2);
      }
    jacobi_eig(h, b, lam, w);
    // Ritz vectors Q W and their images Y W; the residual of the leading ones
    std::vector<double> qw((size_t)N * b);
    for (int32_t j = 0; j < N; ++j)
      for (int c = 0; c < b; ++c) {
        double a1 = 0, a2 = 0;
        for (int k = 0; k < b; ++k) { a1 += q[(size_t)j * b + k] * w[(size_t)k * b + c]; a2 += y[(size_t)j * b + k] * w[(size_t)k * b + c]; }
        qw[(size_t)j * b + c] = a1;
        z[(size_t)j * b + c] = a2;
      }
    double res = 0;
    for (int c = 0; c < FQ_SVD_NPC; ++c) {
      double r2 = 0;
      for (int32_t j = 0; j < N; ++j) { const double r = z[(size_t)j * b + c] - lam[c] * qw[(size_t)j * b + c]; r2 += r * r; }
      res = std::max(res, sqrt(r2));
    }
    p->iterations = it;
    p->lambda0 = lam[0];
    p->residual = lam[0] > 0 ? res / lam[0] : res;
    if (res <= p->o.tol * lam[0]) {
      p->v.assign((size_t)N * FQ_SVD_NPC, 0.);
      for (int32_t j = 0; j < N; ++j) for (int c = 0; c < FQ_SVD_NPC; ++c) p->v[(size_t)j * FQ_SVD_NPC + c] = qw[(size_t)j * b + c];
      lam10.assign(lam.begin(), lam.begin() + FQ_SVD_NPC);
      return 0;
    }
    orthonormalise(z, N, b);
    q.swap(z);
  }
  char m[200];
  snprintf(m, sizeof m, "svd: the residual %.3g (relative to the largest eigenvalue) did not reach %.3g within %d iterations", p->residual, p->o.tol, p->o.max_iter);
  return p->fail(FQ_ELIMIT, m);
}

}  // namespace

extern "C" {

void fq_svd_default_opts(fq_svd_opts_t *o) {
  memset(o, 0, sizeof *o);
  o->max_iter = 2000;
  o->tol = 1e-11;
}

int fq_svd_create(const fq_svd_opts_t *o, fq_svd_t **out) {
  g_create_err.clear();
  if (!out) return FQ_EINVAL;
  *out = nullptr;
  fq_svd_opts_t d;
  fq_svd_default_opts(&d);
  if (o) d = *o;
  if (d.max_iter < 1 || !(d.tol > 0)) { g_create_err = "svd: max_iter must be at least 1 and tol positive"; return FQ_EINVAL; }
  fq_svd *p = new fq_svd;
  p->o = d;
  *out = p;
  return 0;
}

int fq_svd_read_vcf(fq_svd_t *p, const char *path) {
  if (!p || !path) return FQ_EINVAL;
  clear_panel(p);
  const double t0 = now();
  if (int rc = read_vcf(p, path)) { const std::string m = p->err; clear_panel(p); return p->fail(rc, m); }
  p->t_read = now() - t0;
  if (p->N < FQ_SVD_NPC || p->M < FQ_SVD_NPC) {
    char m[200];
    snprintf(m, sizeof m, "svd: %d markers kept and %d samples: the SVD files hold ten components, at least ten of each are needed", p->M, p->N);
    clear_panel(p);
    return p->fail(FQ_EINVAL, m);
  }
  return 0;
}

int fq_svd_set_genotypes(fq_svd_t *p, const int8_t *g, int32_t n_marker, int32_t n_sample, const char *const *chrom, const int32_t *pos, const char *ref, const char *alt,
                         const char *const *samples) {
  if (!p || !g || n_marker < 1 || n_sample < 1) return FQ_EINVAL;
  if (n_marker > FQ_SVD_MAX_MARKERS) return p->fail(FQ_ELIMIT, "svd: more than 2^29 markers");
  clear_panel(p);
  for (size_t i = 0; i < (size_t)n_marker * n_sample; ++i)
    if (g[i] < -1 || g[i] > 2) return p->fail(FQ_EINVAL, "svd: a genotype outside -1 .. 2");
  p->M = n_marker;
  p->N = n_sample;
  p->g.assign(g, g + (size_t)n_marker * n_sample);
  for (int32_t i = 0; i < n_marker; ++i) {
    p->chrom.push_back(chrom ? chrom[i] : "1");
    p->pos.push_back(pos ? pos[i] : i + 1);
    p->bed[p->chrom.back()][p->pos.back()] = std::make_pair(ref ? ref[i] : 'A', alt ? alt[i] : 'C');
  }
  for (int32_t j = 0; j < n_sample; ++j) p->samples.push_back(samples ? samples[j] : "S" + std::to_string(j));
  return 0;
}

int fq_svd_gram(fq_svd_t *p, int32_t *out) {
  if (!p || !out) return FQ_EINVAL;
  if (!p->M) return p->fail(FQ_EINVAL, "svd: no panel set");
  make_gt(p);
  if (p->o.host_eval) { host_gram(p, out, false); return 0; }
  if (int rc = open_device(p)) return rc;
  if (fqdev::svd_gram(p->dd, out)) return p->fail(FQ_ENODEV, std::string("svd: ") + fqdev::last_error());
  return 0;
}

int fq_svd_run(fq_svd_t *p) {
  if (!p) return FQ_EINVAL;
  if (!p->M) return p->fail(FQ_EINVAL, "svd: no panel set");
  if (p->N < FQ_SVD_NPC || p->M < FQ_SVD_NPC) return p->fail(FQ_EINVAL, "svd: the SVD files hold ten components, at least ten markers and ten samples are needed");
  p->ran = false;
  double t0 = now();
  make_gt(p);
  if (p->o.host_eval) host_gram(p, nullptr, true);
  else {
    if (int rc = open_device(p)) return rc;
    if (fqdev::svd_gram(p->dd, nullptr)) return p->fail(FQ_ENODEV, std::string("svd: ") + fqdev::last_error());
  }
  p->t_gram = now() - t0;
  t0 = now();
  std::vector<double> lam;
  if (int rc = iterate(p, lam)) return rc;
  p->t_iter = now() - t0;
  t0 = now();
  const int32_t N = p->N;
  for (int c = 0; c < FQ_SVD_NPC; ++c) {   // the sign: the entry of largest magnitude positive, the first such on ties
    int32_t at = 0;
    for (int32_t j = 1; j < N; ++j) if (fabs(p->v[(size_t)j * FQ_SVD_NPC + c]) > fabs(p->v[(size_t)at * FQ_SVD_NPC + c])) at = j;
    if (p->v[(size_t)at * FQ_SVD_NPC + c] < 0) for (int32_t j = 0; j < N; ++j) p->v[(size_t)j * FQ_SVD_NPC + c] = -p->v[(size_t)j * FQ_SVD_NPC + c];
  }
  p->ud.assign((size_t)p->M * FQ_SVD_NPC, 0.);
  if (p->o.host_eval)
    parallel_for(p->M, n_threads(p), [&](int64_t lo, int64_t hi) {
      for (int64_t i = lo; i < hi; ++i) fq_svd_project(p->gt.data() + i, (size_t)p->m_pad, p->v.data(), N, p->mu[i], p->ud.data() + (size_t)i * FQ_SVD_NPC);
    });
  else if (fqdev::svd_project(p->dd, p->v.data(), p->ud.data())) return p->fail(FQ_ENODEV, std::string("svd: ") + fqdev::last_error());
  p->sigma.assign(FQ_SVD_NPC, 0.);
  for (int c = 0; c < FQ_SVD_NPC; ++c) p->sigma[c] = lam[c] > 0 ? sqrt(lam[c]) : 0.;
  p->t_project = now() - t0;
  p->ran = true;
  return 0;
}

int fq_svd_result(const fq_svd_t *p, fq_svd_result_t *out) {
  if (!p || !out) return FQ_EINVAL;
  memset(out, 0, sizeof *out);
  out->n_marker = p->M;
  out->n_sample = p->N;
  out->t_read = p->t_read;
  if (!p->ran) return p->M ? 0 : FQ_EINVAL;
  out->mu = p->mu.data(); out->ud = p->ud.data(); out->v = p->v.data();
  for (int c = 0; c < FQ_SVD_NPC; ++c) out->sigma[c] = p->sigma[c];
  out->iterations = p->iterations;
  out->residual = p->residual;
  out->t_gram = p->t_gram; out->t_iter = p->t_iter; out->t_project = p->t_project; out->t_write = p->t_write;
  return 0;
}

// WriteSVD (SVDcalculator.cpp:248-279)
int fq_svd_write(fq_svd_t *p, const char *prefix) {
  if (!p || !prefix) return FQ_EINVAL;
  if (!p->ran) return p->fail(FQ_EINVAL, "svd: nothing to write before fq_svd_run");
  const double t0 = now();
  const std::string Prefix(prefix);
  std::ofstream fMu(Prefix + ".mu"), fUD(Prefix + ".UD"), fPC(Prefix + ".V"), fBed(Prefix + ".bed");
  if (!fMu.is_open() || !fUD.is_open() || !fPC.is_open() || !fBed.is_open()) return p->fail(FQ_EIO, "Open file " + Prefix + ".{mu,UD,V,bed} failed!");
  for (int32_t i = 0; i < p->M; ++i) {
    const std::string &chr = p->chrom[i];
    const int beg = p->pos[i] - 1, end = p->pos[i];
    const auto &ra = p->bed[chr][end];
    fMu << chr + ":" + std::to_string(end) << "\t" << p->mu[i] << std::endl;
    fBed << chr << "\t" << beg << "\t" << end << "\t" << ra.first << "\t" << ra.second << std::endl;
    for (int j = 0; j < FQ_SVD_NPC; ++j) fUD << p->ud[(size_t)i * FQ_SVD_NPC + j] << "\t";
    fUD << std::endl;
  }
  for (int32_t k = 0; k < p->N; ++k) {
    fPC << p->samples[k] << "\t";
    for (int i = 0; i < FQ_SVD_NPC; ++i) fPC << p->v[(size_t)k * FQ_SVD_NPC + i] << "\t";
    fPC << std::endl;
  }
  fBed.close(); fMu.close(); fUD.close(); fPC.close();
  if (!fBed || !fMu || !fUD || !fPC) return p->fail(FQ_EIO, "Errors detected when writing to " + Prefix + ".{mu,UD,V,bed} !");
  p->t_write = now() - t0;
  return 0;
}

const char *fq_svd_last_error(const fq_svd_t *p) { return p ? p->err.c_str() : g_create_err.c_str(); }

void fq_svd_destroy(fq_svd_t *p) {
  if (!p) return;
  clear_panel(p);
  if (p->dev) fqdev::state_destroy(p->dev);
  delete p;
}

}  // extern "C"
