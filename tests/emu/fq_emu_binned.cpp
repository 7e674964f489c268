// TEST INFRASTRUCTURE ONLY: fqdev::launch_prep_packed of the host-loop backend with the binned form behind FqPrepPackedArgs::binned (what the tuning key
// filter_binned_min asks for).  Linked into tests/emu/libfq_emu_binned.so (Makefile.binned) in front of fq_emu_backend.cpp, whose own launcher of that
// name -- the direct loop -- is compiled there as launch_prep_packed_direct: the library is the CPU tier's host-loop library in everything else.
#include <cstdlib>
#include <cstring>
#include <string>

#include "fq_backend.h"
#include "fq_emu_binned.h"

namespace fqdev {
int launch_prep_packed_direct(const FqPrepPackedArgs &a);
int launch_prep_packed(const FqPrepPackedArgs &a) {
  if (!a.binned || a.n_reads <= 0 || a.o.filter_thresh == 0) return launch_prep_packed_direct(a);
  if (fq_emu_prep_packed_binned(a)) return -3;
  filter_binned_reads += (uint64_t)a.n_reads;
  return 0;
}
}  // namespace fqdev
