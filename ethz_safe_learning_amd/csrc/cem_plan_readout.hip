// cem_plan_readout.hip — the translation unit of cem_plan_track_kernel (cem_plan_readout.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_PLAN_READOUT_UNIT
#include "cem_plan_readout.h"
