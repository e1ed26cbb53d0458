// cem_population.hip — the translation unit of cem_mean_candidate_kernel (cem_population.h holds it and says why it is compiled apart).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_POPULATION_UNIT
#include "cem_population.h"
