// TEST INFRASTRUCTURE ONLY: the VCF reader, the host loops and the writers of `svd` (fq_svd.cpp, fq_svd.h) under AddressSanitizer / UBSan, as a program
// of its own.  tests/test_svd.py builds and runs it:
//     make && ./svd_check <out dir> <panel.vcf[.gz]>...
// Each panel is read, decomposed by the host loops (two threads) and written to <out dir>/<k> (.mu, .UD, .V, .bed; k counts from 0); then a VCF that ends
// in a refusal goes through the reader, and a panel goes in from memory.  The device launchers fq_svd.cpp refers to are stubs here: the host loops
// never call them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastquick_amd.h"
#include "fq_svd.h"

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
}  // namespace fqdev
extern "C" int fq_host_cpus(void) { return 2; }

static int bad(const char *what, fq_svd_t *p) {
  fprintf(stderr, "svd_check: %s: %s\n", what, fq_svd_last_error(p));
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: svd_check OUT_DIR PANEL.vcf[.gz]...\n"); return 2; }
  fq_svd_opts_t o;
  fq_svd_default_opts(&o);
  o.host_eval = 1;
  o.host_threads = 2;
  fq_svd_t *p = nullptr;
  if (fq_svd_create(&o, &p)) return bad("create", nullptr);
  fq_svd_result_t r;
  for (int k = 2; k < argc; ++k) {
    if (fq_svd_read_vcf(p, argv[k])) return bad("read", p);
    if (fq_svd_run(p)) return bad("run", p);
    if (fq_svd_result(p, &r)) return bad("result", p);
    const std::string pre = std::string(argv[1]) + "/" + std::to_string(k - 2);
    if (fq_svd_write(p, pre.c_str())) return bad("write", p);
    printf("svd_check: %s: %d markers, %d samples, %d iterations, residual %.3g, sigma_0 %.17g\n", argv[k], r.n_marker, r.n_sample, r.iterations, r.residual, r.sigma[0]);
  }
  // a record the reference reads out of bounds on (a GT with one allele): refused, and the object takes another panel afterwards
  const std::string vcf = std::string(argv[1]) + "/one_allele.vcf";
  FILE *f = fopen(vcf.c_str(), "w");
  if (!f) return 2;
  fprintf(f, "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT");
  for (int j = 0; j < 10; ++j) fprintf(f, "\tS%d", j);
  fprintf(f, "\n1\t100\t.\tA\tC\t.\t.\t.\tGT");
  for (int j = 0; j < 10; ++j) fprintf(f, "\t%s", j == 7 ? "1" : "0/1");
  fprintf(f, "\n");
  fclose(f);
  if (fq_svd_read_vcf(p, vcf.c_str()) == 0 || !strstr(fq_svd_last_error(p), "line 3")) { fprintf(stderr, "svd_check: the one-allele GT was not refused by line\n"); return 1; }
  // a panel from memory: 12 markers x 11 samples, the Gram matrix against the plain loop, then the whole decomposition
  const int M = 12, N = 11;
  std::vector<int8_t> g((size_t)M * N);
  unsigned s = 7;
  for (auto &x : g) { s = s * 1664525u + 1013904223u; x = (int8_t)((s >> 24) % 4) - 1; }
  if (fq_svd_set_genotypes(p, g.data(), M, N, nullptr, nullptr, nullptr, nullptr, nullptr)) return bad("set_genotypes", p);
  std::vector<int32_t> a((size_t)N * N);
  if (fq_svd_gram(p, a.data())) return bad("gram", p);
  int n_bad = 0;
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < N; ++k) {
      int32_t want = 0;
      for (int i = 0; i < M; ++i) want += g[(size_t)i * N + j] * g[(size_t)i * N + k];
      n_bad += want != a[(size_t)j * N + k];
    }
  if (fq_svd_run(p)) return bad("run (memory)", p);
  if (fq_svd_write(p, (std::string(argv[1]) + "/mem").c_str())) return bad("write (memory)", p);
  fq_svd_destroy(p);
  printf("svd_check: Gram entries, %d differ\n", n_bad);
  return n_bad ? 1 : 0;
}
