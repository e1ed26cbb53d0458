// cem_elite_carry.hip — the translation unit of cem_elite_keep_kernel and cem_elite_inject_kernel (cem_elite_carry.h holds them and says why they are compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_ELITE_CARRY_UNIT
#include "cem_elite_carry.h"
