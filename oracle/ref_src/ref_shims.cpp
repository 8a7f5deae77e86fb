// TEST INFRASTRUCTURE ONLY: extern "C" drivers over this project's stand-ins for GSL, FFTW3 and ParseHeader
// (oracle/ref_shim/), so that tests/test_reference_runs.py can hold each against an independent truth: MT19937's
// published first word and the oracle's own generator, numpy.fft, the committed parameter texts.
#include <cstring>
#include <string>
#include <vector>

#include "ParseHeader.hh"
#include <fmt/ranges.h>
#include "fftw3.h"
#include "gsl/gsl_rng.h"

extern "C" void shim_mt_words(unsigned long seed, int n, unsigned int *words, double *uniform) {
    gsl_rng *r = gsl_rng_alloc(gsl_rng_mt19937);
    gsl_rng_set(r, seed);
    for (int i = 0; i < n; i++) words[i] = (unsigned int) gsl_rng_get(r);
    gsl_rng_set(r, seed);
    for (int i = 0; i < n; i++) uniform[i] = gsl_rng_uniform(r);
    gsl_rng_free(r);
}

// rank 1: n1 points; rank 2: n0 x n1; planned on NULL arrays as the reference does, executed in place
extern "C" int shim_dft(int rank, int n0, int n1, int sign, double *data) {
    fftw_plan p = rank == 1 ? fftw_plan_dft_1d(n1, NULL, NULL, sign, FFTW_PATIENT) : fftw_plan_dft_2d(n0, n1, NULL, NULL, sign, FFTW_PATIENT);
    if (!p) return 1;
    fftw_execute_dft(p, (fftw_complex *) data, (fftw_complex *) data);
    fftw_destroy_plan(p);
    return 0;
}

// parses `text` with the symbols src/parameters.cpp registers (same names, types and MUST_DEFINE flags are the
// caller's: `must` lists the keys that must be defined, separated by blanks); writes "key=value\n" lines of a fixed
// subset into `out`.  Returns 0, or 1 with the complaint in `out`.
extern "C" int shim_parse(const char *text, const char *must, char *out, int outlen) {
    ParseHeader ph;
    double boxsize = 0, pk_scale = 0, pk_norm = 0, pk_sigma = 0, pk_sigma_ratio = 0, f_cluster = 1, pk_smooth = 0, index = 1000,
           z_initial = 0, target_z = 0, k_cutoff = 1, f_NL = 0, n_s = 1, omega_m = 1;
    long long np = 0;
    int numblock = 2, cpd = 0, qdensity = 0, qoneslab = -1, seed = 0, fix = 0, qonemode = 0, qplt = 0, rescale = 0, dio = 0, version = -1,
        corner = 0;
    std::string icformat;
    fs::path pkfile, outdir, densfile = "density{:d}", pltfile;
    std::vector<int> one_mode = {0, 0, 0};
    std::string m = std::string(" ") + must + " ";
    auto md = [&](const char *k) { return m.find(std::string(" ") + k + " ") != std::string::npos; };
#define S(key, var) ph.installscalar(key, var, md(key))
    S("BoxSize", boxsize); S("ZD_Pk_scale", pk_scale); S("NP", np); S("ZD_NumBlock", numblock); S("CPD", cpd);
    S("ZD_qdensity", qdensity); S("ZD_qoneslab", qoneslab); S("ZD_Seed", seed); S("ZD_Pk_norm", pk_norm);
    S("ZD_Pk_sigma", pk_sigma); S("ZD_Pk_sigma_ratio", pk_sigma_ratio); S("ZD_f_cluster", f_cluster);
    S("ZD_Pk_smooth", pk_smooth); S("ZD_qPk_fix_to_mean", fix); S("ZD_Pk_filename", pkfile);
    S("ZD_Pk_powerlaw_index", index); S("InitialConditionsDirectory", outdir); S("ZD_density_filename", densfile);
    S("InitialRedshift", z_initial); S("ZD_qonemode", qonemode); S("ZD_qPLT", qplt); S("ZD_PLT_filename", pltfile);
    S("ZD_qPLT_rescale", rescale); S("ZD_PLT_target_z", target_z); S("ZD_k_cutoff", k_cutoff); S("ZD_f_NL", f_NL);
    S("ZD_n_s", n_s); S("Omega_M", omega_m); S("ICFormat", icformat); S("AllowDirectIO", dio); S("ZD_Version", version);
    S("ZD_CornerModes", corner);
#undef S
    ph.installvector("ZD_one_mode", one_mode, md("ZD_one_mode"));
    std::string err = ph.ParseText(text);
    std::string o = err;
    if (err.empty())
        o = fmt::format(
           "BoxSize={}\nNP={}\nZD_NumBlock={}\nCPD={}\nZD_Seed={}\nZD_Pk_sigma={}\nZD_Pk_sigma_ratio={}\nZD_Pk_smooth={}\n"
           "ZD_Pk_powerlaw_index={}\nZD_k_cutoff={}\nZD_f_cluster={}\nZD_f_NL={}\nICFormat={}\nZD_Pk_filename={}\n"
           "InitialConditionsDirectory={}\nZD_PLT_filename={}\nZD_qPLT={}\nZD_qPLT_rescale={}\nZD_Version={}\nZD_CornerModes={}\n"
           "ZD_qdensity={}\nZD_qoneslab={}\nZD_qonemode={}\nZD_one_mode={}\n",
           boxsize, np, numblock, cpd, seed, pk_sigma, pk_sigma_ratio, pk_smooth, index, k_cutoff, f_cluster, f_NL, icformat,
           pkfile.string(), outdir.string(), pltfile.string(), qplt, rescale, version, corner, qdensity, qoneslab, qonemode,
           fmt::join(one_mode, " "));
    strncpy(out, o.c_str(), outlen - 1);
    out[outlen - 1] = 0;
    return err.empty() ? 0 : 1;
}
