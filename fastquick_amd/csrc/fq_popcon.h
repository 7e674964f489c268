// fq_popcon.h -- the mixture likelihood of `FASTQuick pop+con` (VerifyBamID2's ContaminationEstimator), stated once for host and device.
//
// Restates FullLLKFunc::ComputeMixLLKs (VerifyBamID/ContaminationEstimator.h:206-281) with its helpers getConditionalBaseLK (:142-196),
// InitialGF (:198-204) and Phred (:55-57), in double and in the reference's operation order.  The term a base adds to a genotype pair's sum,
//     log((alpha * E[g1][c] + (1 - alpha) * E[g2][c]) * phred(q) + (alpha * N[g1][c] + (1 - alpha) * N[g2][c]) * (1 - phred(q))),
// depends on the base's class c (ref / alt / other), its quality character q, the pair (g1, g2) and alpha alone: an evaluation builds the table of
// these terms once (fq_pc_term, the reference's own expression) and the sums over a marker's bases add the same doubles in the same order as the
// reference's loop.  The host loop (fq_popcon.cpp: the --host_eval evaluator, the yardstick) and the kernels below walk the same packed pileup
// with the same routines; the device's exp / log / pow are its own library's, which is the whole of the difference.
#pragma once
#include "fq_common.h"
#include <cmath>
#include <cstdint>

#define FQ_PC_MAXPC 8          // principal components an estimator takes (the command line keeps vb2Main.cpp's 4)
#define FQ_PC_MAXQ 85          // distinct quality characters of a pileup: a base's byte is quality slot * 3 + class, below 255
#define FQ_PC_TERMS (FQ_PC_MAXQ * 3 * 9)
#define FQ_PC_PAD 16           // a marker's bytes begin at a multiple of 16: lanes read them as 16-byte pieces
#define FQ_PC_CLS_REF 0
#define FQ_PC_CLS_ALT 1
#define FQ_PC_CLS_OTHER 2
#define FQ_PC_GROUPS 7         // markers a wavefront holds at a time: nine lanes (one per genotype pair) each, lane 63 idle
#define FQ_PC_BLOCK 256
#define FQ_PC_PER_BLOCK (FQ_PC_GROUPS * (FQ_PC_BLOCK / 64))

// class of a pileup character against the marker's alt allele (getConditionalBaseLK's three tests, in its order)
FQ_HD int fq_pc_class(char base, char alt) {
  if (base == '.' || base == ',') return FQ_PC_CLS_REF;
  const int b = (unsigned char)base, a = (unsigned char)alt;   // toupper of the "C" locale, as the reference runs under
  const int bu = b >= 'a' && b <= 'z' ? b - 32 : b, au = a >= 'a' && a <= 'z' ? a - 32 : a;
  return bu == au ? FQ_PC_CLS_ALT : FQ_PC_CLS_OTHER;
}
// getConditionalBaseLK(base of class c, genotype g, is_error)
FQ_HD double fq_pc_cond(int c, int g, bool is_error) {
  if (!is_error) {
    if (g == 0) return c == FQ_PC_CLS_REF ? 1 : 0;
    if (g == 1) return c == FQ_PC_CLS_OTHER ? 0 : 0.5;
    return c == FQ_PC_CLS_ALT ? 1 : 0;
  }
  if (g == 0) return c == FQ_PC_CLS_REF ? 0 : c == FQ_PC_CLS_ALT ? 1. / 3. : 2. / 3.;
  if (g == 1) return c == FQ_PC_CLS_OTHER ? 2. / 3. : 1. / 6.;
  return c == FQ_PC_CLS_REF ? 1. / 3. : c == FQ_PC_CLS_ALT ? 0 : 2. / 3.;
}
// the term of one base: quality character q (a char: signed, as tmpQual[j] - 33 is), class c, genotypes g1 / g2
FQ_HD double fq_pc_term(double alpha, int q, int c, int g1, int g2) {
  const double ph = pow(10.0, (double)(q - 33) / -10.0);
  return log((alpha * fq_pc_cond(c, g1, true) + (1. - alpha) * fq_pc_cond(c, g2, true)) * ph +
             (alpha * fq_pc_cond(c, g1, false) + (1. - alpha) * fq_pc_cond(c, g2, false)) * (1 - ph));
}
FQ_HD void fq_pc_gf(double af, double *gf) {   // InitialGF
  if (af < 0.00005) af = 0.00005;
  if (af > 0.99995) af = 0.99995;
  gf[0] = (1 - af) * (1 - af);
  gf[1] = 2 * (af) * (1 - af);
  gf[2] = af * af;
}
FQ_HD double fq_pc_af(const double *ud, const double *pc, int n_pc, double mean) {
  double af = 0.;
  for (int k = 0; k < n_pc; ++k) af += ud[k] * pc[k];
  af += mean;
  af /= 2.0;
  return af;
}

// The packed pileup of an estimate, in marker order of the .bed (host arrays on the host side, device arrays on the device).
struct FqPcPile {
  int32_t n_marker, n_pc, n_q, known_af;
  const uint32_t *depth;     // bases of marker i (0: absent from the pileup, or an empty line)
  const uint64_t *off;       // first byte of marker i in `code` (a multiple of FQ_PC_PAD); off[n_marker] = bytes in all
  const uint8_t *code;       // quality slot * 3 + class per base, pileup order
  const uint8_t *skip;       // 1: the marker adds nothing (absent, empty, or outside avgDepth +- 3 sdDepth under the sanity check)
  const int8_t *q_of_slot;   // the quality character of a slot
  const double *ud, *mean, *af;   // n_marker x n_pc, n_marker, n_marker (known allele frequencies; read when known_af)
};
// a point of the likelihood: pc1[FQ_PC_MAXPC], pc2[FQ_PC_MAXPC], alpha
#define FQ_PC_POINT (2 * FQ_PC_MAXPC + 1)

// the skip rule of ComputeMixLLKs (:218-232): size_t against double, as there
FQ_HD bool fq_pc_skip(uint32_t depth, bool sanity, double avg, double sd) {
  if (depth == 0) return true;
  const size_t d = depth;
  return sanity && (d < (avg - 3 * sd) || d > (avg + 3 * sd));
}

// table[(slot * 3 + class) * 9 + g1 * 3 + g2], entry t
FQ_HD double fq_pc_table_entry(const FqPcPile &P, double alpha, int t) {
  const int g = t % 9, code = t / 9;
  return fq_pc_term(alpha, P.q_of_slot[code / 3], code % 3, g / 3, g % 3);
}
// one genotype pair's weighted likelihood of marker i: exp(sum of terms) * GF[g1] * GF2[g2]
FQ_HD double fq_pc_pair(const FqPcPile &P, const double *table, const double *pt, int i, int g) {
  double af1, af2;
  if (P.known_af) af1 = af2 = P.af[i];
  else {
    af1 = fq_pc_af(P.ud + (size_t)i * P.n_pc, pt, P.n_pc, P.mean[i]);
    af2 = fq_pc_af(P.ud + (size_t)i * P.n_pc, pt + FQ_PC_MAXPC, P.n_pc, P.mean[i]);
  }
  double gf[3], gf2[3];
  fq_pc_gf(af1, gf);
  fq_pc_gf(af2, gf2);
  const uint8_t *c = P.code + P.off[i];
  const uint32_t d = P.depth[i];
  double s = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (uint32_t j = 0; j < d; j += 16) {   // sixteen bases a load (the marker's bytes are padded to sixteen)
    const uint4 v = *(const uint4 *)(c + j);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t n = d - j < 16 ? d - j : 16;
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b)
      if (b < n) s += table[((w[b >> 2] >> (8 * (b & 3))) & 0xff) * 9 + g];
  }
#else
  for (uint32_t j = 0; j < d; ++j) s += table[c[j] * 9 + g];
#endif
  return exp(s) * gf[g / 3] * gf2[g % 3];
}
// log(markerLK) or 0 from the nine pairs' values, added in g1-major order
FQ_HD double fq_pc_marker_close(const double *v9) {
  double lk = 0;
  for (int g = 0; g < 9; ++g) lk += v9[g];
  return lk > 0 ? log(lk) : 0.;
}
// host loop over one marker
inline double fq_pc_marker_host(const FqPcPile &P, const double *table, const double *pt, int i) {
  if (P.skip[i]) return 0.;
  double v[9];
  for (int g = 0; g < 9; ++g) v[g] = fq_pc_pair(P, table, pt, i, g);
  return fq_pc_marker_close(v);
}

#if defined(__HIPCC__) && defined(FQ_PC_KERNELS)
// ---- kernels (launched from fq_device.hip) ----
// once per estimate: a thread per padded byte finds its marker in the scanned offsets and writes class + quality slot; the first n_marker
// threads also write the skip flags
struct FqPcPrepArgs {
  int32_t n_marker, sanity;
  double avg, sd;
  const uint32_t *depth;
  const uint64_t *off;      // scan of the padded depths
  const uint64_t *raw_off;  // scan of the depths: marker i's characters in base / qual
  const char *base, *qual, *alt;
  const uint8_t *slot_of_q; // 256 entries
  uint8_t *code, *skip;
};
__global__ void __launch_bounds__(256) k_pc_prepare(FqPcPrepArgs a, uint64_t n_bytes) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < (uint64_t)a.n_marker) a.skip[t] = fq_pc_skip(a.depth[t], a.sanity != 0, a.avg, a.sd) ? 1 : 0;
  if (t >= n_bytes) return;
  int lo = 0, hi = a.n_marker;      // the marker whose padded range holds byte t: off[lo] <= t < off[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.off[mid] <= t) lo = mid; else hi = mid;
  }
  const uint64_t j = t - a.off[lo];
  uint8_t c = 0;
  if (j < a.depth[lo]) {
    const uint64_t r = a.raw_off[lo] + j;
    c = (uint8_t)(a.slot_of_q[(uint8_t)a.qual[r]] * 3 + fq_pc_class(a.base[r], a.alt[lo]));
  }
  a.code[t] = c;
}
// once per evaluation: blockIdx.y is the point.  The block builds its point's term table in LDS; a wavefront then takes seven markers at a
// time, nine lanes a marker (a lane per genotype pair walks the marker's bases in order), the nine values are added in g1-major order by
// shuffles and log(markerLK) -- or 0 -- goes to out[point * n_marker + marker].  Every marker's slot is written.
__global__ void __launch_bounds__(FQ_PC_BLOCK) k_pc_llk(FqPcPile P, const double *pts, double *out) {
  __shared__ double table[FQ_PC_TERMS];
  const double *pt = pts + (size_t)blockIdx.y * FQ_PC_POINT;
  const double alpha = pt[2 * FQ_PC_MAXPC];
  for (int t = threadIdx.x; t < P.n_q * 27; t += FQ_PC_BLOCK) table[t] = fq_pc_table_entry(P, alpha, t);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane / 9, g = lane - grp * 9;
  double *o = out + (size_t)blockIdx.y * P.n_marker;
  for (int base = blockIdx.x * FQ_PC_PER_BLOCK; base < P.n_marker; base += gridDim.x * FQ_PC_PER_BLOCK) {
    const int i = base + wave * FQ_PC_GROUPS + grp;
    const bool live = lane < 63 && i < P.n_marker;
    double v = 0;
    if (live && !P.skip[i]) v = fq_pc_pair(P, table, pt, i, g);
    double lk = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) lk += __shfl(v, (grp * 9 + k) & 63, 64);
    if (live && g == 0) o[i] = (!P.skip[i] && lk > 0) ? log(lk) : 0.;
  }
}
// the sums of the P rows of `out`, one block a row: thread t adds elements t, t + 256, ... in order, then a tree over the 256 partial sums
// (a fixed shape: the same input gives the same bits)
__global__ void __launch_bounds__(256) k_pc_sum(const double *out, int n_marker, double *sums) {
  __shared__ double part[256];
  const double *o = out + (size_t)blockIdx.x * n_marker;
  double s = 0;
  for (int i = threadIdx.x; i < n_marker; i += 256) s += o[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = part[0];
}
#endif

namespace fqdev {
struct State;
// launchers of the kernels above (fq_device.hip), on the bound state's stream
struct FqPcPrepHost {      // host arrays of an estimate, uploaded and packed by pc_prepare
  int32_t n_marker, n_pc, n_q, known_af, sanity;
  double avg, sd;
  const uint32_t *depth; const char *base, *qual, *alt; uint64_t n_chars;
  const uint8_t *slot_of_q; const int8_t *q_of_slot;
  const double *ud, *mean, *af;
};
struct PcDev;                                               // the device arrays of an estimate
PcDev *pc_prepare(const FqPcPrepHost &h, int max_points);   // nullptr on failure (last_error())
void pc_free(PcDev *d);
// sums[0..n) = the likelihood at pts[0..n) (FQ_PC_POINT doubles each); n <= max_points.  Points and sums travel through pinned memory the kernels
// read and write in place; one wait on the stream.
int pc_llk(PcDev *d, const double *pts, int n, double *sums);
int pc_marker_llk(PcDev *d, const double *pt, double *per_marker);   // the per-marker values of one point (tests)
}  // namespace fqdev
