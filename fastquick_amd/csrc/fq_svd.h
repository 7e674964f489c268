// fq_svd.h -- the SVD files of `FASTQuick pop+con --RefVCF` (VerifyBamID2's SVDcalculator::ProcessRefVCF), stated once for host and device.
//
// The reference centres the markers x samples genotype matrix by its float row means and runs Eigen's JacobiSVD<MatrixXf> on it
// (VerifyBamID/SVDcalculator.cpp:195-236); the files hold the ten leading components.  Here the same decomposition comes from the exact integer
// Gram matrix of the genotypes:
//     A = G^T G                      int32, exact                                   (fq_svd_dot: k_svd_gram, MFMA i8)
//     t_j = sum_i mu_i g_ij,  q = sum_i mu_i^2                                      (fq_svd_t_term: k_svd_tq)
//     C_jk = A_jk - (t_j + t_k) + q  = (X^T X)_jk,  X_ij = g_ij - mu_i, in double   (fq_svd_centre: k_svd_centre)
//     Y = C Q                        the step of the block subspace iteration       (fq_svd_apply: k_svd_apply)
//     UD_ic = sum_j g_ij v_jc - mu_i sum_j v_jc  = (X V)_ic                         (fq_svd_project: k_svd_project)
// The host loops (fq_svd.cpp: --host_eval, the CPU tier) and the kernels below run these statements over the same sample-major int8 matrix
// gt[n_pad][m_pad] (sample j's markers contiguous, zero beyond N and M: a zero adds nothing to an integer product).
#pragma once
#include "fq_common.h"
#include <cstdint>
#include <cstddef>

#define FQ_SVD_NPC 10          // components WriteSVD prints (SVDcalculator.cpp:263, :270)
#define FQ_SVD_BLOCK_MAX 32    // width of the iterated block: min(N, 32)
#define FQ_SVD_TILE 32         // samples a Gram tile is wide and markers a matrix instruction contracts
#define FQ_SVD_MAX_MARKERS (1 << 29)   // 4 * M fits int32: a product of two genotypes is at most 4

// mu_i = float(sum_j g_ij) / float(N): Eigen's rowwise().mean() on the float matrix (the row sum of at most 2^24 small integers is exact in float)
FQ_HD double fq_svd_mean(int32_t row_sum, int32_t n_sample) { return (double)((float)row_sum / (float)n_sample); }
// A_jk: the product of two samples' marker rows
FQ_HD int32_t fq_svd_dot(const int8_t *a, const int8_t *b, int64_t m) {
  int32_t s = 0;
  for (int64_t i = 0; i < m; ++i) s += (int32_t)a[i] * (int32_t)b[i];
  return s;
}
FQ_HD double fq_svd_t_term(double mu, int8_t g) { return mu * (double)g; }
// (the sum t_j + t_k first: C_jk and C_kj are then the same bits)
FQ_HD double fq_svd_centre(int32_t a, double tj, double tk, double q) { return ((double)a - (tj + tk)) + q; }
// Y_jc = sum_k C_jk Q_kc: row j of C (n doubles), Q row-major n x b
FQ_HD double fq_svd_apply(const double *c_row, const double *q, int32_t n, int32_t b, int32_t c) {
  double s = 0;
  for (int32_t k = 0; k < n; ++k) s += c_row[k] * q[(size_t)k * b + c];
  return s;
}
// the ten values of marker i: g points at gt[0][i], sample j's value lies `stride` bytes further per sample; v row-major n x 10
FQ_HD void fq_svd_project(const int8_t *g, size_t stride, const double *v, int32_t n, double mu, double *out) {
  double acc[FQ_SVD_NPC], sum[FQ_SVD_NPC];
  for (int c = 0; c < FQ_SVD_NPC; ++c) acc[c] = sum[c] = 0;
  for (int32_t j = 0; j < n; ++j) {
    const double gj = (double)g[(size_t)j * stride];
    const double *vj = v + (size_t)j * FQ_SVD_NPC;
    for (int c = 0; c < FQ_SVD_NPC; ++c) { acc[c] += gj * vj[c]; sum[c] += vj[c]; }
  }
  for (int c = 0; c < FQ_SVD_NPC; ++c) out[c] = acc[c] - mu * sum[c];
}

#if defined(__HIPCC__) && defined(FQ_SVD_KERNELS)
// ---- kernels (launched from fq_device.hip) ----
typedef int fq_svd_v4i __attribute__((ext_vector_type(4)));
typedef int fq_svd_v16i __attribute__((ext_vector_type(16)));
struct FqSvdGramArgs {
  const int8_t *gt;      // [n_pad][m_pad]
  int32_t *a;            // [n_pad][n_pad], zero on entry
  int32_t n_tiles;       // n_pad / 32
  int32_t n_split;       // gridDim.y: blocks that share a tile pair's markers
  int64_t m_pad;         // a multiple of 32
};
// A block takes the pair of 32-sample tiles (tj <= tk) numbered blockIdx.x and slice blockIdx.y of the markers; its four wavefronts take a quarter of the
// slice each, 32 markers an instruction: lane (r = lane & 31, h = lane >> 5) hands v_mfma_i32_32x32x32_i8 sixteen consecutive markers of sample
// tj * 32 + r as A and of sample tk * 32 + r as B -- whichever marker the instruction takes byte e of half h for, it is the same one in A and in B, and
// the sum over markers has no order.  The sixteen results of a lane are column lane & 31, rows (reg & 3) + 8 * (reg >> 2) + 4 * h of the tile; they are
// added to a[] (and to the mirrored entry of a tile off the diagonal) with integer atomics: exact, whatever the order of the blocks.
// Bounds: rows < n_tiles * 32 = n_pad; a lane's last byte is chunk * 32 + 16 * h + 15 < m_pad.
__global__ void __launch_bounds__(256) k_svd_gram(FqSvdGramArgs p) {
  int tj = 0, rem = (int)blockIdx.x;
  while (rem >= p.n_tiles - tj) { rem -= p.n_tiles - tj; ++tj; }
  const int tk = tj + rem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int64_t n_chunks = p.m_pad / FQ_SVD_TILE, workers = (int64_t)p.n_split * 4, wid = (int64_t)blockIdx.y * 4 + wave;
  const int64_t per = (n_chunks + workers - 1) / workers;
  const int64_t c0 = wid * per, c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
  const int8_t *pa = p.gt + (size_t)(tj * FQ_SVD_TILE + r) * p.m_pad + 16 * h;
  const int8_t *pb = p.gt + (size_t)(tk * FQ_SVD_TILE + r) * p.m_pad + 16 * h;
  fq_svd_v16i acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0;
  for (int64_t ch = c0; ch < c1; ++ch) {
    const fq_svd_v4i a = *(const fq_svd_v4i *)(pa + ch * FQ_SVD_TILE);
    const fq_svd_v4i b = *(const fq_svd_v4i *)(pb + ch * FQ_SVD_TILE);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
  }
  if (c0 >= c1) return;
  const size_t n_pad = (size_t)p.n_tiles * FQ_SVD_TILE;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const size_t row = (size_t)tj * FQ_SVD_TILE + (e & 3) + 8 * (e >> 2) + 4 * h, col = (size_t)tk * FQ_SVD_TILE + r;
    atomicAdd(p.a + row * n_pad + col, acc[e]);
    if (tj != tk) atomicAdd(p.a + col * n_pad + row, acc[e]);
  }
}
// block j < n: t_j; block n: q.  Thread t adds markers t, t + 256, ... in order, then a tree over the 256 partial sums (a fixed shape: the same bits every run)
__global__ void __launch_bounds__(256) k_svd_tq(const int8_t *gt, int64_t m_pad, int64_t m, int32_t n, const double *mu, double *tq) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double s = 0;
  if (j < n) { const int8_t *g = gt + (size_t)j * m_pad; for (int64_t i = threadIdx.x; i < m; i += 256) s += fq_svd_t_term(mu[i], g[i]); }
  else for (int64_t i = threadIdx.x; i < m; i += 256) s += mu[i] * mu[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) tq[j] = part[0];
}
__global__ void __launch_bounds__(256) k_svd_centre(const int32_t *a, size_t n_pad, int32_t n, const double *tq, double *c) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n) return;
  const size_t j = t / n, k = t % n;
  c[t] = fq_svd_centre(a[j * n_pad + k], tq[j], tq[k], tq[n]);
}
// a block of 32 x 8 threads: threadIdx.x is the column of Q, threadIdx.y one of eight rows of C
__global__ void __launch_bounds__(256) k_svd_apply(const double *c, const double *q, int32_t n, int32_t b, double *y) {
  const int32_t j = blockIdx.x * 8 + threadIdx.y, col = threadIdx.x;
  if (j >= n || col >= b) return;
  y[(size_t)j * b + col] = fq_svd_apply(c + (size_t)j * n, q, n, b, col);
}
// a thread per marker: one pass over the int8 matrix (neighbouring threads read neighbouring bytes of a sample's row)
__global__ void __launch_bounds__(128) k_svd_project(const int8_t *gt, int64_t m_pad, int64_t m, int32_t n, const double *v, const double *mu, double *ud) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= m) return;
  fq_svd_project(gt + i, (size_t)m_pad, v, n, mu[i], ud + (size_t)i * FQ_SVD_NPC);
}
#endif

namespace fqdev {
struct State;
// launchers of the kernels above (fq_device.hip), on the bound state's stream
struct SvdDev;   // the device arrays of a decomposition
// gt: host [n_pad][m_pad] (n_pad, m_pad multiples of 32, zero beyond n and m); mu: m doubles.  nullptr on failure (last_error())
SvdDev *svd_upload(const int8_t *gt, int32_t n, int32_t n_pad, int64_t m, int64_t m_pad, const double *mu);
void svd_free(SvdDev *d);
int svd_gram(SvdDev *d, int32_t *a_out);    // A, t, q and C on the device; a_out (n x n, may be nullptr) receives A
int svd_apply(SvdDev *d, const double *q, int32_t b, double *y);   // y = C q, both n x b row-major on the host; one wait
int svd_project(SvdDev *d, const double *v, double *ud);           // v: n x 10, ud: m x 10
}  // namespace fqdev
