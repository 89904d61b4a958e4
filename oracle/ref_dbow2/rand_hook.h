// TEST INFRASTRUCTURE ONLY: force-included (-include) in front of every translation unit of oracle/_ref/ref_dbow2. It routes
// the rand() behind DUtils::Random to the driver, which hands out a supplied list of integers, without touching the
// reference's sources. The standard headers that name rand themselves are included first, so the macro cannot reach them.
#ifndef REF_DBOW2_RAND_HOOK_H
#define REF_DBOW2_RAND_HOOK_H

#include <cstdlib>
#ifdef __cplusplus
#include <algorithm>
#include <random>
extern "C" int ref_dbow2_rand(void);
#else
int ref_dbow2_rand(void);
#endif
#define rand ref_dbow2_rand

#endif
