// the three-role kernel's one-step agent-loop instantiations at APAD = 8 --
// the C3 agent loop's K = 1 (trio_agent8_list, mgn_units.h): their
// own unit, built without machine LICM (madigan_amd/build.py)
#include "mgn_launch_impl.h"
MGN_DEFINE_UNIT(a8k1)
#ifdef MGN_ITERSTAMP
// diagnostic build: this unit's copy of the iteration stamps (the one-step
// launches run here; mgn_diag_iter reads mgn_launch_a8t.hip's)
extern "C" int mgn_diag_iter_k1(unsigned long long* h) {
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(mgn::g_iter), 256 * 64 * sizeof(unsigned long long)) != hipSuccess)
    return 1;
  static unsigned long long z[256 * 64] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(mgn::g_iter), z, sizeof(z)) != hipSuccess;
}
#endif
