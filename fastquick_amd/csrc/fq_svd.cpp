// fq_svd.cpp -- `FASTQuick pop+con --RefVCF` (VerifyBamID2's SVDcalculator) around the statements of fq_svd.h: the subcommand `svd`.
//
// Host side: the serial VCF reader (its statement for one record stands in fq_svd_host.h, shared with the chunked reader of fq_vcf.cpp; SVDcalculator::ReadVcf, SVDcalculator.cpp:18-193, with libVcf's tokenising of a record: libVcfFile.cpp:473-530, :910-940,
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
#include "fq_svd_host.h"

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

using namespace fqsvd;

void clear_panel(fq_svd *p) {
  if (p->dd) { if (p->dev && !fqdev::bind(p->dev)) fqdev::svd_free(p->dd); p->dd = nullptr; }
  p->M = p->N = 0;
  p->g.clear(); p->samples.clear(); p->chrom.clear(); p->pos.clear(); p->bed.clear();
  p->gt.clear(); p->c.clear();
  p->ran = false;
  p->rs = fq_svd_read_stats_t{};
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
  bool have_header = false;
  RecState S;
  S.path = path;
  int64_t &line_no = S.line_no;
  size_t at = 0;
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
        header_samples(ln, n, p->samples);
        have_header = true;
        if (p->samples.empty()) return p->fail(FQ_EINVAL, std::string("No individual genotype information exist in the input VCF file ") + path);
        p->N = (int32_t)p->samples.size();
        continue;
      }
      return p->fail(FQ_EINVAL, "Header line is not found : #CHROM..." + S.where());
    }
    if (n == 0) break;   // (the reference's reader ends at an empty line)
    if (const int rc = fq_svd_record(p, S, ln, n); rc < 0) return rc;
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
  o->chunk_bytes = (int64_t)256 << 20;
}

int fq_svd_create(const fq_svd_opts_t *o, fq_svd_t **out) {
  g_create_err.clear();
  if (!out) return FQ_EINVAL;
  *out = nullptr;
  fq_svd_opts_t d;
  fq_svd_default_opts(&d);
  if (o) d = *o;
  if (d.max_iter < 1 || !(d.tol > 0)) { g_create_err = "svd: max_iter must be at least 1 and tol positive"; return FQ_EINVAL; }
  if (d.reader < 0 || d.reader > 2 || d.chunk_bytes < 0) { g_create_err = "svd: reader is 0 (serial), 1 (kernels) or 2 (host loops), chunk_bytes not negative"; return FQ_EINVAL; }
  if (!d.chunk_bytes) d.chunk_bytes = (int64_t)256 << 20;
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

int fq_svd_read_stats(const fq_svd_t *p, fq_svd_read_stats_t *out) {
  if (!p || !out) return FQ_EINVAL;
  *out = p->rs;
  return 0;
}

int fq_svd_panel(const fq_svd_t *p, int8_t *g, int32_t *pos, const char **chrom, const char **samples) {
  if (!p) return FQ_EINVAL;
  if (g && !p->g.empty()) memcpy(g, p->g.data(), p->g.size());
  for (int32_t i = 0; i < p->M; ++i) { if (pos) pos[i] = p->pos[i]; if (chrom) chrom[i] = p->chrom[i].c_str(); }
  for (int32_t j = 0; j < p->N; ++j) if (samples) samples[j] = p->samples[j].c_str();
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
