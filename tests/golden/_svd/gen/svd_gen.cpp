// svd_gen.cpp -- generator of tests/golden/_svd: drives VerifyBamID2's SVDcalculator (compiled from the reference tree, see README.md) over a panel
// VCF and leaves the four files fastquick_amd's `svd` is held to.  Never part of the product, never run by a test.
//
//   svd_gen PANEL.vcf[.gz]          SVDcalculator::ProcessRefVCF: writes PANEL.vcf[.gz].UD / .mu / .V / .bed, prints the wall time of the call
//   svd_gen --time M N              Eigen's JacobiSVD<MatrixXf> (ComputeThinU | ComputeThinV, the call of SVDcalculator.cpp:218) on a mean-centred
//                                   M x N matrix of values in {0, 1, 2}: its wall time alone
//
// SimplePileupViewer.cpp (BAM pileup, BAQ) needs htslib and is not compiled; SVDcalculator refers to none of its members.  The BGZF reader of
// statgen's InputFile needs samtools' bgzf.c, which the reference tree does not carry: its entry points are defined below and end the run, so
// the generator reads plain and gzip files (what make_fixtures.py writes).
#include "SVDcalculator.h"
#include "Eigen/Dense"
#include "bgzf.h"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static void no_bgzf() { fprintf(stderr, "svd_gen: BGZF input is not supported by the generator\n"); exit(2); }
extern "C" {
BGZF *bgzf_fdopen(int, const char *) { no_bgzf(); return nullptr; }
BGZF *bgzf_open(const char *, const char *) { no_bgzf(); return nullptr; }
int bgzf_close(BGZF *) { no_bgzf(); return 0; }
ssize_t bgzf_read(BGZF *, void *, ssize_t) { no_bgzf(); return 0; }
ssize_t bgzf_write(BGZF *, const void *, ssize_t) { no_bgzf(); return 0; }
int64_t bgzf_seek(BGZF *, int64_t, int) { no_bgzf(); return 0; }
int bgzf_check_EOF(BGZF *) { no_bgzf(); return 0; }
}

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "--time")) {
    const int M = atoi(argv[2]), N = atoi(argv[3]);
    Eigen::MatrixXf X(M, N);
    unsigned s = 12345;
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < N; ++j) { s = s * 1664525u + 1013904223u; X(i, j) = (float)((s >> 24) % 3); }
    Eigen::VectorXf mu = X.rowwise().mean();
    for (int i = 0; i < M; ++i) for (int j = 0; j < N; ++j) X(i, j) -= mu(i);
    const double t0 = now();
    Eigen::JacobiSVD<Eigen::MatrixXf> svd(X, Eigen::ComputeThinU | Eigen::ComputeThinV);
    const double t1 = now();
    printf("JacobiSVD<MatrixXf> %d x %d: %.2f s (sigma_0 %g)\n", M, N, t1 - t0, (double)svd.singularValues()(0));
    return 0;
  }
  if (argc != 2) { fprintf(stderr, "usage: svd_gen PANEL.vcf[.gz] | svd_gen --time M N\n"); return 2; }
  SVDcalculator calc;
  const double t0 = now();
  calc.ProcessRefVCF(argv[1]);
  fprintf(stderr, "svd_gen: ProcessRefVCF %.2f s\n", now() - t0);
  return 0;
}
