// zd_plt.h — the PLT eigenmode table computed on the GPU (zd_kernels_plt.hip; zd_make_eigenmodes, include/zeldovich_hip.h):
// what the host layer and the kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace zd {

constexpr double PLT_ALPHA = 2.0;  // Ewald splitting parameter of the product table
constexpr int PLT_SHELLS   = 4;    // R, m in [-4, 4]^3: omitted terms < 1e-20

struct PltConst {
    int n;           // points per side of the table: k = 2 pi m / n
    double inv4a2;   // 1 / (4 alpha^2)
    double self;     // 4 alpha^3 / (3 sqrt pi)
};

// vectors of the half shell of [-s, s]^3: the first non-zero of (R_x, R_y, R_z) is positive
constexpr int plt_half_shell(int s) { return ((2 * s + 1) * (2 * s + 1) * (2 * s + 1) - 1) / 2; }

// alpha -> PltConst and A(R) | B(R) of the half shell in the kernels' order (std::erfc, on the host)
PltConst plt_const(int n, double alpha);
std::vector<double> plt_shell_table(double alpha, int shells);

// rows [kx0, kx0 + nkx) of the table into out[(ikx - kx0)][iky][ikz][4]; tab: device image of plt_shell_table(alpha, PLT_SHELLS)
int launch_plt_modes(const PltConst &c, const double *tab, int kx0, int nkx, double *out, hipStream_t st);
#ifdef ZD_TESTING
// the six distinct elements xx, yy, zz, xy, xz, yz of D at nmodes signed wavenumbers; shells 3, 4 or 5
int launch_test_plt_matrix(const PltConst &c, int shells, const double *tab, long long nmodes, const int *m_xyz, double *out6, hipStream_t st);
#endif

}  // namespace zd
