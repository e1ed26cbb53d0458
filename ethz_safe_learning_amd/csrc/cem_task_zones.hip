// cem_task_zones.hip — the translation unit of cem_task_zones_kernel (cem_task_zones.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_TASK_ZONES_UNIT
#include "cem_task_zones.h"
