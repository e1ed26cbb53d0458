// cem_task_reference.hip — the translation unit of cem_task_reference_kernel (cem_task_reference.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_TASK_REFERENCE_UNIT
#include "cem_task_reference.h"
