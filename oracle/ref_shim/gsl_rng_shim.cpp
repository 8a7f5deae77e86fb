// TEST INFRASTRUCTURE ONLY: MT19937 behind the GSL interface (see gsl/gsl_rng.h).
#include <cstdint>
#include <cstdlib>

#include "gsl/gsl_rng.h"

struct gsl_rng_type_shim {
    const char *name;
};
struct gsl_rng_shim {
    uint32_t mt[624];
    int mti;
};

static const gsl_rng_type_shim mt19937_type = {"mt19937"};
extern "C" {
const gsl_rng_type *gsl_rng_mt19937 = &mt19937_type;
}

extern "C" void gsl_rng_set(const gsl_rng *rc, unsigned long int seed) {
    gsl_rng *r = const_cast<gsl_rng *>(rc);
    if (seed == 0) seed = 4357;  // GSL's default seed for this generator
    r->mt[0] = (uint32_t) (seed & 0xffffffffUL);
    for (int i = 1; i < 624; i++)
        r->mt[i] = 1812433253U * (r->mt[i - 1] ^ (r->mt[i - 1] >> 30)) + (uint32_t) i;
    r->mti = 624;
}

extern "C" gsl_rng *gsl_rng_alloc(const gsl_rng_type *T) {
    if (T != gsl_rng_mt19937) abort();
    gsl_rng *r = (gsl_rng *) malloc(sizeof(gsl_rng));
    if (!r) abort();
    gsl_rng_set(r, 0);
    return r;
}

extern "C" unsigned long int gsl_rng_get(const gsl_rng *rc) {
    gsl_rng *r = const_cast<gsl_rng *>(rc);
    uint32_t *mt = r->mt;
    if (r->mti >= 624) {
        for (int k = 0; k < 624; k++) {
            uint32_t y = (mt[k] & 0x80000000U) | (mt[(k + 1) % 624] & 0x7fffffffU);
            mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
        }
        r->mti = 0;
    }
    uint32_t y = mt[r->mti++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680U;
    y ^= (y << 15) & 0xefc60000U;
    y ^= y >> 18;
    return y;
}

extern "C" double gsl_rng_uniform(const gsl_rng *r) { return gsl_rng_get(r) / 4294967296.0; }

extern "C" void gsl_rng_free(gsl_rng *r) { free(r); }
