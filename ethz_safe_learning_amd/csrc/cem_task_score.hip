// cem_task_score.hip — the translation unit of cem_task_score_kernel (cem_task_score.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_TASK_SCORE_UNIT
#include "cem_task_score.h"
