// the three-role kernel's n-step instantiations at APAD = 2 (trio_nst_list,
// mgn_units.h): their own unit for their own flags
// (madigan_amd/build.py UNIT_FLAGS)
#include "mgn_launch_impl.h"
MGN_DEFINE_UNIT(a2nst)
