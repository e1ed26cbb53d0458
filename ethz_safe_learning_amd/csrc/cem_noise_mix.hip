// cem_noise_mix.hip — the translation unit of cem_mix_action_noise_kernel (cem_noise_mix.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_NOISE_MIX_UNIT
#include "cem_noise_mix.h"
