// TEST INFRASTRUCTURE ONLY: the host readers and the host evaluator of pop+con (fq_popcon.cpp, fq_popcon.h) under AddressSanitizer / UBSan, as a
// program of its own.  tests/test_popcon.py builds and runs it:
//     make && ./popcon_check <svd prefix> <pileup> <golden file> <num_pc> <out prefix>
// It reads the fixture, evaluates the likelihood at the golden's points (bit for bit), runs the estimate with the sanity check disabled and writes
// the three files.  The device launchers fq_popcon.cpp refers to are stubs here: the host evaluator never calls them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "fastquick_amd.h"
#include "fq_popcon.h"

namespace fqdev {
State *state_create(int) { return nullptr; }
void state_destroy(State *) {}
int bind(State *) { return -3; }
const char *last_error() { return "no device in this build"; }
PcDev *pc_prepare(const FqPcPrepHost &, int) { return nullptr; }
void pc_free(PcDev *) {}
int pc_llk(PcDev *, const double *, int, double *) { return -3; }
int pc_marker_llk(PcDev *, const double *, double *) { return -3; }
}  // namespace fqdev
extern "C" int fq_host_cpus(void) { return 2; }

static int bad(const char *what, fq_popcon_t *p) {
  fprintf(stderr, "popcon_check: %s: %s\n", what, fq_popcon_last_error(p));
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 6) { fprintf(stderr, "usage: popcon_check SVD_PREFIX PILEUP GOLDEN NUM_PC OUT_PREFIX\n"); return 2; }
  const int k = atoi(argv[4]);
  fq_popcon_opts_t o;
  fq_popcon_default_opts(&o);
  o.num_pc = k;
  o.disable_sanity_check = 1;
  o.host_eval = 1;
  o.host_threads = 2;
  fq_popcon_t *p = nullptr;
  if (fq_popcon_create(argv[1], nullptr, nullptr, nullptr, &o, &p)) return bad("create", nullptr);
  if (fq_popcon_set_pileup_file(p, argv[2])) return bad("pileup", p);
  std::ifstream g(argv[3]);
  std::string line;
  int n_points = 0, n_bad = 0;
  while (std::getline(g, line)) {
    std::stringstream ss(line);
    std::string w;
    ss >> w;
    if (w != "point") continue;
    std::vector<double> pt(2 * k + 1);
    double want = 0;
    ss >> w;
    for (int i = 0; i < k; ++i) ss >> pt[i];
    ss >> w;
    for (int i = 0; i < k; ++i) ss >> pt[k + i];
    ss >> w >> pt[2 * k] >> w >> want;
    double got = 0;
    if (fq_popcon_llk(p, pt.data(), 1, &got)) return bad("llk", p);
    ++n_points;
    if (memcmp(&got, &want, 8)) { ++n_bad; fprintf(stderr, "popcon_check: point %d: %.17g, golden %.17g\n", n_points, got, want); }
  }
  fq_popcon_result_t r;
  if (fq_popcon_run(p)) return bad("run", p);
  if (fq_popcon_result(p, &r)) return bad("result", p);
  if (fq_popcon_write(p, argv[5])) return bad("write", p);
  // a second pileup through the array entry on the same object, then the per-marker values
  const int32_t marker[5] = {0, 0, 3, r.n_marker - 1, 3};
  const char base[5] = {'.', 'N', ',', 'a', 'T'}, qual[5] = {'I', '!', '~', '5', 'I'};
  if (fq_popcon_set_pileup_arrays(p, marker, base, qual, 5)) return bad("arrays", p);
  std::vector<double> pt(2 * k + 1, 0.01);
  pt[2 * k] = 0.2;
  std::vector<double> per(r.n_marker);
  if (fq_popcon_marker_llk(p, pt.data(), per.data())) return bad("marker_llk", p);
  fq_popcon_destroy(p);
  printf("popcon_check: %d points, %d differ; alpha %.17g, %lld evaluations, %d markers used\n", n_points, n_bad, r.alpha, (long long)r.n_eval, r.markers_used);
  return n_bad || n_points == 0 ? 1 : 0;
}
