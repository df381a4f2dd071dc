// the three-role kernel for one-asset envs with n-step rings
// (trio_one_list, mgn_units.h): its own unit for its own flags
// (madigan_amd/build.py UNIT_FLAGS)
#include "mgn_launch_impl.h"
MGN_DEFINE_UNIT(a1tnst)
