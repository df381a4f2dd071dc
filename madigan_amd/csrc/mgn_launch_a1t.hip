// the three-role kernel for one-asset envs (trio_one_list,
// mgn_units.h: two lanes per env and role, the second a pad): its own
// unit, compiled beside the others
#include "mgn_launch_impl.h"
MGN_DEFINE_UNIT(a1t)
