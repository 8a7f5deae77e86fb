// zd_glass.h — what zd_kernels_glass.hip (the interpolation object and its kernels) shares with zd_capi_interp.cpp (zd_plan_interp,
// zd_displace): the refusals of a particle load, the object of one sweep of a tiled load, the memory it takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zeldovich_hip.h"

namespace zdglass {

// per z weight j of a delivered plane: the range of the sorted particles whose z cell takes that weight from the plane
struct PlaneJob {
    unsigned start[4], count[4];
};

constexpr long long MAX_SWEEP = (1LL << 31) - 1;  // particles of one object: sorted slots are 32-bit
constexpr int BYTES_PER_PARTICLE = 84;            // u = p N (24), permutation (4), six sums (48), its share of the result pieces (6) + slack

// what zd_interp_create and zd_displace refuse about a load before the GPU is touched (the message names the argument); NULL: nothing
const char *load_refusal(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, int64_t tile, char *buf, size_t cap);
// bins of the counting sort's histogram (4 bytes each, held while an object is created)
long long hist_bins(int64_t ppd);
// the object of the particles [first, first + count) of the load tiled `tile` times (definition: zd_kernels_glass.hip); no checks of the load
int create(int64_t ppd, int32_t icformat, int32_t order, int64_t npart, const double *pos_xyz, int64_t tile, int64_t first, int64_t count,
           zd_interp **out);
void shape(const zd_interp *it, int64_t *ppd, int32_t *icformat);

}  // namespace zdglass
