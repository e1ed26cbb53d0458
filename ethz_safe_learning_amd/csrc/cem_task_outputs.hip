// cem_task_outputs.hip — the translation unit of cem_task_outputs_kernel (cem_task_outputs.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_TASK_OUTPUTS_UNIT
#include "cem_task_outputs.h"
