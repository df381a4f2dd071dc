// launchers for APAD = 64, portfolio-weight input (see mgn_launch.h)
#include "mgn_launch_impl.h"
MGN_DEFINE_UNIT(a64w)
