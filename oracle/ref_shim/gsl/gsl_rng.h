/* TEST INFRASTRUCTURE ONLY.  This project's stand-in for the four GSL entry points the reference program calls
 * (gsl_rng_alloc / gsl_rng_set / gsl_rng_uniform / gsl_rng_free on gsl_rng_mt19937).  Written here behind GSL's
 * interface; no GSL code.  MT19937 (Matsumoto & Nishimura) with the 2002 init_genrand seeding, seed 0 -> 4357 as GSL
 * documents; gsl_rng_uniform = word / 2^32.  Checked against the published first word of seed 5489 and the
 * oracle's own mt19937 (tests/test_reference_runs.py). */
#ifndef ZD_SHIM_GSL_RNG_H
#define ZD_SHIM_GSL_RNG_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsl_rng_type_shim gsl_rng_type;
typedef struct gsl_rng_shim gsl_rng;

extern const gsl_rng_type *gsl_rng_mt19937;

gsl_rng *gsl_rng_alloc(const gsl_rng_type *T);
void gsl_rng_set(const gsl_rng *r, unsigned long int seed);
unsigned long int gsl_rng_get(const gsl_rng *r);
double gsl_rng_uniform(const gsl_rng *r);
void gsl_rng_free(gsl_rng *r);

#ifdef __cplusplus
}
#endif
#endif
