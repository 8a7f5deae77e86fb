// zeldovich_main.cpp — `zeldovich <param_file>`: the drop-in command line of the reference
// (src/zeldovich.cpp:848-1032) on top of the MI355X library.  Host C++ only; everything heavy is
// behind the C ABI of include/zeldovich_hip.h.
//
// Same external surface: one argument, same parameter keys, ic_{z*CPD/PPD} files of ICFormat records
// under InitialConditionsDirectory, optional density file, progress on stderr, exit code 0 / 1.
// Differences that are deliberate and documented in DESIGN.md: no FFTW wisdom file, no block files
// (DISK mode is replaced by HBM residency + z-residue streaming), planes may be produced out of z
// order and are therefore placed with pwrite at their final offset instead of being appended.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <map>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/zeldovich_hip.h"

namespace fs = std::filesystem;

struct Writer {
    zd_params p;
    fs::path dir;
    int recsize = 0;
    int64_t plane_bytes = 0;
    std::map<int, int> fds;  // ic file index -> fd
    int dens_fd = -1;
    size_t bytes_written = 0;
    double seconds = 0;
    // ZD_SelfCheck: the sites (z, y, x), and the record / density the callback delivered at each of them
    std::vector<int64_t> sites;
    std::vector<unsigned char> site_rec;
    std::vector<float> site_dens;
    std::vector<int> site_seen;

    // first z stored in file `f`: smallest z with z*cpd/ppd == f   (output.cpp:208)
    int64_t first_z_of_file(int f) const {
        if (p.cpd <= 0) return 0;  // CPD <= 0: z*cpd/ppd == 0 for every plane, everything lands in ic_0 (as in the reference)
        int64_t z = ((int64_t) f * p.ppd + p.cpd - 1) / p.cpd;
        while (z > 0 && (z - 1) * p.cpd / p.ppd == f) z--;
        while (z * p.cpd / p.ppd < f) z++;
        return z;
    }
    int fd_for(int f) {
        auto it = fds.find(f);
        if (it != fds.end()) return it->second;
        const fs::path fn = dir / ("ic_" + std::to_string(f));
        // planes are placed with pwrite, so a file is opened once per run: truncate whatever an earlier (longer) run left
        int fd = open(fn.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) {
            fprintf(stderr, "Could not open output file \"%s\"\n", fn.c_str());
            exit(1);
        }
        fds[f] = fd;
        return fd;
    }
    static int callback(void *user, int64_t z, int64_t n, const void *records, const float *density) {
        Writer *w = (Writer *) user;
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < w->site_seen.size(); i++) {
            if (w->sites[3 * i] != z) continue;
            const int64_t at = w->sites[3 * i + 1] * w->p.ppd + w->sites[3 * i + 2];
            if (records) memcpy(w->site_rec.data() + i * w->recsize, (const unsigned char *) records + at * w->recsize, w->recsize);
            if (density) w->site_dens[i] = density[at];
            w->site_seen[i] = 1;
        }
        if (records) {
            const int f = (int) (z * w->p.cpd / w->p.ppd);
            // with ZD_qoneslab only one plane is written; the reference appends it at offset 0
            const int64_t zrel = w->p.qoneslab >= 0 ? 0 : z - w->first_z_of_file(f);
            const int fd       = w->fd_for(f);
            const size_t nb    = (size_t) n * w->recsize;
            if (pwrite(fd, records, nb, (off_t) (zrel * w->plane_bytes)) != (ssize_t) nb) {
                fprintf(stderr, "Short write on ic_%d\n", f);
                return 1;
            }
            w->bytes_written += nb;
        }
        if (density && w->dens_fd >= 0) {
            const size_t nb    = (size_t) n * sizeof(float);
            const int64_t zrel = w->p.qoneslab >= 0 ? 0 : z;
            if (pwrite(w->dens_fd, density, nb, (off_t) (zrel * (int64_t) nb)) != (ssize_t) nb) return 1;
            w->bytes_written += nb;
        }
        w->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
    void close_all() {
        for (auto &kv : fds) close(kv.second);
        if (dens_fd >= 0) close(dens_fd);
    }
};

// SetupOutputDir: src/output.cpp:236-251
static void setup_output_dir(const fs::path &dir) {
    if (fs::exists(dir)) {
        for (const auto &entry : fs::directory_iterator(dir)) {
            if (entry.is_regular_file()) {
                const std::string fn = entry.path().filename().string();
                if (fn.compare(0, 3, "ic_") == 0 || fn.compare(0, 10, "zeldovich.") == 0) fs::remove(entry.path());
            }
        }
    }
    fs::create_directories(dir);
}

static double cube(double a) { return a == 0.0 ? 0.0 : a * a * a; }

// ZD_Pk_measured_filename: band power of the realised modes (zd_measure_power), one line per non-empty |k| shell
static int write_measured_power(const char *path, const zd_params &p, const zd_pk &pk, const double *eig, int64_t eig_ppd) {
    const int64_t nb = zd_power_nbins(p.ppd, 1);
    std::vector<int64_t> count(nb);
    std::vector<double> sk(nb), sd(nb), si(nb), sq(nb), sv(nb);
    if (zd_measure_power(&p, &pk, eig, eig_ppd, 1, nb, count.data(), sk.data(), sd.data(), si.data(), sq.data(), sv.data())) return 1;
    FILE *f = fopen(path, "w");
    if (!f) {
        fprintf(stderr, "Could not open band-power file \"%s\"\n", path);
        return 1;
    }
    fprintf(f, "# k_mean count P_measured P_input disp_power vel_power\n");
    double worst = 0.0;
    for (int64_t b = 0; b < nb; b++) {
        if (count[b] == 0) continue;
        const double n = (double) count[b];
        fprintf(f, "%.17g %lld %.17g %.17g %.17g %.17g\n", sk[b] / n, (long long) count[b], sd[b] / n, si[b] / n, sq[b] / n, sv[b] / n);
        if (si[b] > 0) worst = std::max(worst, fabs(sd[b] / si[b] - 1.0) * sqrt(n));
    }
    fclose(f);
    fprintf(stderr, "Measured band power written to %s: worst |P_measured / P_input - 1| sqrt(count) over the bins is %g\n", path, worst);
    return 0;
}

// ZD_SelfCheck = n.  THE SITES: a splitmix64 stream started at ZD_Seed gives three draws per site, (z, y, x) = draw mod PPD each, in that
// order, site after site; site 1 then takes z = (z of site 0 + 1) mod PPD, so that for n >= 2 the sites lie on two different z residues
// of every stream factor >= 2 (stream factors divide PPD); with ZD_qoneslab every site takes z = ZD_qoneslab.
static std::vector<int64_t> self_check_sites(const zd_params &p, int n) {
    uint64_t state = (uint64_t) p.seed;
    auto next = [&]() {
        uint64_t v = (state += 0x9E3779B97F4A7C15ULL);
        v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ULL;
        v = (v ^ (v >> 27)) * 0x94D049BB133111EBULL;
        return v ^ (v >> 31);
    };
    std::vector<int64_t> s(3 * (size_t) n);
    for (auto &v : s) v = (int64_t) (next() % (uint64_t) p.ppd);
    if (n >= 2) s[3] = (s[0] + 1) % p.ppd;
    if (p.qoneslab >= 0)
        for (int i = 0; i < n; i++) s[3 * i] = p.qoneslab;
    return s;
}

// the delivered records at the sites against zd_direct_sum; returns non-zero if the check fails or cannot be made
static int self_check(const Writer &w, const zd_param_strings &s, const zd_pk &pk, const double *eig, int64_t eig_ppd) {
    const zd_params &p = w.p;
    const int n = (int) w.site_seen.size();
    std::vector<double> sum(7 * (size_t) n), rec(7 * (size_t) n, NAN);
    if (zd_direct_sum(&p, &pk, eig, eig_ppd, n, w.sites.data(), sum.data())) return 1;
    const bool have_rec = w.recsize > 0, have_vel = p.icformat == ZD_FMT_RVZEL || p.icformat == ZD_FMT_RVDOUBLEZEL, have_dens = p.qdensity != 0;
    double qmax = 0, dmax = 0, worst = 0, worst_dens = 0;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < 3; j++) qmax = std::max(qmax, fabs(sum[7 * i + j]));
        dmax = std::max(dmax, fabs(sum[7 * i + 6]));
    }
    for (int i = 0; i < n; i++) {
        if (!w.site_seen[i]) {
            fprintf(stderr, "self-check: plane z = %lld was never delivered\n", (long long) w.sites[3 * i]);
            return 1;
        }
        const unsigned char *r = w.site_rec.data() + (size_t) i * w.recsize;
        // records hold (z, y, x) components: d[3] (+ v[3]) behind the 8-byte lattice index, ZelSimple d[3] alone; float32 or float64
        const bool f64 = p.icformat == ZD_FMT_RVDOUBLEZEL || p.icformat == ZD_FMT_ZEL;
        const size_t off = p.icformat == ZD_FMT_ZELSIMPLE ? 0 : 8;
        for (int j = 0; have_rec && j < (have_vel ? 6 : 3); j++) {
            double v;
            if (f64) {
                memcpy(&v, r + off + 8 * j, 8);
            } else {
                float f;
                memcpy(&f, r + off + 4 * j, 4);
                v = f;
            }
            const int col = j < 3 ? 2 - j : 3 + (5 - j);  // (qz, qy, qx, vz, vy, vx) -> qx, qy, qz, vx, vy, vz
            rec[7 * i + col] = v;
            worst = std::max(worst, fabs(v - sum[7 * i + col]) / qmax);
        }
        if (have_dens) {  // the density plane is float32 in every format: the direct sum is rounded to it before the comparison
            rec[7 * i + 6] = w.site_dens[i];
            worst_dens = std::max(worst_dens, fabs((double) w.site_dens[i] - (double) (float) sum[7 * i + 6]) / dmax);
        }
    }
    if (s.SelfCheck_filename[0]) {
        FILE *f = fopen(s.SelfCheck_filename, "w");
        if (!f) {
            fprintf(stderr, "Could not open self-check file \"%s\"\n", s.SelfCheck_filename);
            return 1;
        }
        fprintf(f, "# z y x | record: qx qy qz vx vy vz density (nan: not delivered) | direct sum: qx qy qz vx vy vz density\n");
        for (int i = 0; i < n; i++) {
            fprintf(f, "%lld %lld %lld", (long long) w.sites[3 * i], (long long) w.sites[3 * i + 1], (long long) w.sites[3 * i + 2]);
            for (int j = 0; j < 7; j++) fprintf(f, " %.17g", rec[7 * i + j]);
            for (int j = 0; j < 7; j++) fprintf(f, " %.17g", sum[7 * i + j]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    fprintf(stderr, "self-check: %d sites, max |record - direct sum| / max|q| = %.3g", n, worst);
    if (have_dens) fprintf(stderr, ", max |density - direct sum| / max|density| = %.3g", worst_dens);
    fprintf(stderr, " (ZD_SelfCheck_tol = %g)\n", s.SelfCheck_tol);
    if (!(worst <= s.SelfCheck_tol) || !(worst_dens <= s.SelfCheck_tol)) {
        fprintf(stderr, "self-check FAILED: the delivered records differ from the direct summation over the modes\n");
        return 1;
    }
    return 0;
}

// ZD_LPT_SelfCheck, ZD_LPT_SelfCheck_tol, ZD_LPT_SelfCheck_filename, ZD_LPT_Pk_filename (optional, not in the reference; ZD_q2LPT runs):
// keys without a member in zd_param_strings, read with zd_param_file_string.  A numeric key is parsed strictly.
struct LptKeys {
    int selfcheck = 0;
    double tol = 0;
    char selfcheck_filename[1024] = "", pk_filename[1024] = "";
};

static int refuse(const char *key, const char *value, const char *why) {
    fprintf(stderr, "Invalid Parameters given: %s = %s %s\n", key, value, why);
    return 1;
}

// non-zero (one line on stderr) if the file cannot be read or a key's value is refused
static int read_lpt_keys(const char *path, LptKeys &k) {
    char v[1024], old[1024];
    if (zd_param_file_string(path, "ZD_LPT_SelfCheck", v, sizeof(v))) return 1;
    if (v[0]) {
        char *end = nullptr;
        const long n = strtol(v, &end, 10);
        if (end == v || *end) return refuse("ZD_LPT_SelfCheck", v, "is not an integer");
        if (n < 0 || n > 64) return refuse("ZD_LPT_SelfCheck", v, "must lie in 0 ... 64 (sites; 0 = off)");
        k.selfcheck = (int) n;
    }
    if (zd_param_file_string(path, "ZD_LPT_SelfCheck_tol", v, sizeof(v))) return 1;
    if (v[0]) {
        char *end = nullptr;
        k.tol = strtod(v, &end);
        if (end == v || *end) return refuse("ZD_LPT_SelfCheck_tol", v, "is not a number");
        if (!(k.tol >= 0)) return refuse("ZD_LPT_SelfCheck_tol", v, "must be >= 0");
    }
    if (zd_param_file_string(path, "ZD_LPT_SelfCheck_filename", k.selfcheck_filename, sizeof(k.selfcheck_filename)) ||
        zd_param_file_string(path, "ZD_LPT_Pk_filename", k.pk_filename, sizeof(k.pk_filename)) ||
        zd_param_file_string(path, "ZD_SelfCheck", old, sizeof(old)))
        return 1;
    if (k.selfcheck > 0 && old[0] && strtol(old, nullptr, 10) != 0)
        return refuse("ZD_LPT_SelfCheck", v[0] ? v : "n", "does not run together with ZD_SelfCheck: one check keeps the records at the sites");
    if (zd_param_file_string(path, "ZD_q2LPT", old, sizeof(old))) return 1;
    if ((k.selfcheck > 0 || k.pk_filename[0]) && strtol(old, nullptr, 10) != 1) {
        fprintf(stderr, "Invalid Parameters given: %s needs ZD_q2LPT = 1 (it sums the orders of an LPT run)\n",
                k.selfcheck > 0 ? "ZD_LPT_SelfCheck" : "ZD_LPT_Pk_filename");
        return 1;
    }
    return 0;
}

// ZD_LPT_Pk_filename: band power of the three orders (zd_lpt_power), one line per non-empty |k| shell
static int write_lpt_power(const char *path, const zd_params &p, const zd_pk &pk) {
    const int64_t nb = zd_power_nbins(p.ppd, 1);
    std::vector<int64_t> count(nb);
    std::vector<double> sums(8 * (size_t) nb);
    if (zd_lpt_power(&p, &pk, 1, nb, count.data(), sums.data())) return 1;
    FILE *f = fopen(path, "w");
    if (!f) {
        fprintf(stderr, "Could not open LPT band-power file \"%s\"\n", path);
        return 1;
    }
    fprintf(f, "# k_mean count P_input P_measured disp1_power disp2_power disp3_power disp_power vel_power\n");
    for (int64_t b = 0; b < nb; b++) {
        if (count[b] == 0) continue;
        const double n = (double) count[b];
        fprintf(f, "%.17g %lld", sums[8 * b] / n, (long long) count[b]);
        for (int j = 1; j < 8; j++) fprintf(f, " %.17g", sums[8 * b + j] / n);
        fprintf(f, "\n");
    }
    fclose(f);
    fprintf(stderr, "LPT band power written to %s\n", path);
    return 0;
}

// ZD_LPT_SelfCheck = n: the delivered records at the sites of self_check_sites against zd_lpt_direct_sum; returns non-zero if the
// check fails or cannot be made
static int lpt_self_check(const Writer &w, const LptKeys &k, const zd_pk &pk) {
    const zd_params &p = w.p;
    const int n = (int) w.site_seen.size();
    std::vector<double> sum(18 * (size_t) n), rec(6 * (size_t) n, NAN);
    if (zd_lpt_direct_sum(&p, &pk, n, w.sites.data(), sum.data())) return 1;
    const bool have_vel = p.icformat == ZD_FMT_RVZEL || p.icformat == ZD_FMT_RVDOUBLEZEL;
    const bool f64 = p.icformat == ZD_FMT_RVDOUBLEZEL || p.icformat == ZD_FMT_ZEL;
    const double tol = k.tol > 0 ? k.tol : (f64 ? 1e-10 : 1e-6);  // the defaults of ZD_SelfCheck_tol
    auto total = [&](int i, int col) { return sum[18 * i + col] + sum[18 * i + 6 + col] + sum[18 * i + 12 + col]; };
    double qmax = 0, m2 = 0, m3 = 0, worst = 0;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) {
            qmax = std::max(qmax, fabs(total(i, j)));
            m2   = std::max(m2, fabs(sum[18 * i + 6 + j]));
            m3   = std::max(m3, fabs(sum[18 * i + 12 + j]));
        }
    for (int i = 0; i < n; i++) {
        if (!w.site_seen[i]) {
            fprintf(stderr, "lpt self-check: plane z = %lld was never delivered\n", (long long) w.sites[3 * i]);
            return 1;
        }
        const unsigned char *r = w.site_rec.data() + (size_t) i * w.recsize;
        const size_t off = p.icformat == ZD_FMT_ZELSIMPLE ? 0 : 8;  // (the record layout: self_check)
        for (int j = 0; j < (have_vel ? 6 : 3); j++) {
            double v;
            if (f64) {
                memcpy(&v, r + off + 8 * j, 8);
            } else {
                float f;
                memcpy(&f, r + off + 4 * j, 4);
                v = f;
            }
            const int col = j < 3 ? 2 - j : 3 + (5 - j);  // (qz, qy, qx, vz, vy, vx) -> qx, qy, qz, vx, vy, vz
            rec[6 * i + col] = v;
            worst = std::max(worst, fabs(v - total(i, col)) / qmax);
        }
    }
    if (k.selfcheck_filename[0]) {
        FILE *f = fopen(k.selfcheck_filename, "w");
        if (!f) {
            fprintf(stderr, "Could not open LPT self-check file \"%s\"\n", k.selfcheck_filename);
            return 1;
        }
        fprintf(f, "# z y x | record: qx qy qz vx vy vz (nan: not delivered) | direct sum, order 1: qx qy qz vx vy vz | order 2 | order 3\n");
        for (int i = 0; i < n; i++) {
            fprintf(f, "%lld %lld %lld", (long long) w.sites[3 * i], (long long) w.sites[3 * i + 1], (long long) w.sites[3 * i + 2]);
            for (int j = 0; j < 6; j++) fprintf(f, " %.17g", rec[6 * i + j]);
            for (int j = 0; j < 18; j++) fprintf(f, " %.17g", sum[18 * i + j]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    fprintf(stderr, "lpt self-check: %d sites, max |record - direct sum| / max|q| = %.3g, max|psi2| / max|q| = %.3g, max|psi3| / max|q| = %.3g "
                    "(ZD_LPT_SelfCheck_tol = %g)\n", n, worst, m2 / qmax, m3 / qmax, tol);
    if (!(worst <= tol)) {
        fprintf(stderr, "lpt self-check FAILED: the delivered records differ from the direct summation over the three orders\n");
        return 1;
    }
    return 0;
}

// ZD_Glass_filename, ZD_Glass_tile, ZD_Glass_order, ZD_Glass_output (optional, not in the reference): displacements and velocities for
// an off-lattice particle load (zd_displace) instead of the lattice's ic_* files; read with zd_param_file_string
struct GlassKeys {
    char filename[1024] = "", output[1024] = "";
    long tile = 1, order = 3;
    std::vector<double> pos;  // the load: (x, y, z) per particle
};

// non-zero (one line on stderr) if the file cannot be read, a key's value is refused or the load cannot be used
static int read_glass_keys(const char *path, GlassKeys &k) {
    char tile[1024], order[1024];
    if (zd_param_file_string(path, "ZD_Glass_filename", k.filename, sizeof(k.filename)) || zd_param_file_string(path, "ZD_Glass_tile", tile, sizeof(tile)) ||
        zd_param_file_string(path, "ZD_Glass_order", order, sizeof(order)) || zd_param_file_string(path, "ZD_Glass_output", k.output, sizeof(k.output)))
        return 1;
    if (!k.filename[0]) {
        const char *other = tile[0] ? "ZD_Glass_tile" : order[0] ? "ZD_Glass_order" : k.output[0] ? "ZD_Glass_output" : nullptr;
        if (other) {
            fprintf(stderr, "Invalid Parameters given: %s needs ZD_Glass_filename (the particle load it applies to)\n", other);
            return 1;
        }
        return 0;
    }
    char *end = nullptr;
    if (tile[0]) {
        k.tile = strtol(tile, &end, 10);
        if (end == tile || *end) return refuse("ZD_Glass_tile", tile, "is not an integer");
        if (k.tile < 1 || k.tile > 65536) return refuse("ZD_Glass_tile", tile, "must lie in 1 ... 65536");
    }
    if (order[0]) {
        k.order = strtol(order, &end, 10);
        if (end == order || *end) return refuse("ZD_Glass_order", order, "is not an integer");
        if (k.order != 1 && k.order != 3) return refuse("ZD_Glass_order", order, "must be 1 (trilinear) or 3 (cubic Lagrange)");
    }
    std::error_code ec;
    const uintmax_t size = fs::file_size(k.filename, ec);
    if (ec) {
        fprintf(stderr, "Invalid Parameters given: ZD_Glass_filename = %s cannot be read\n", k.filename);
        return 1;
    }
    if (size == 0 || size % 24) {
        fprintf(stderr, "Invalid Parameters given: ZD_Glass_filename = %s holds %llu bytes: float64 triples (x, y, z) make a multiple of 24\n", k.filename,
                (unsigned long long) size);
        return 1;
    }
    k.pos.resize(size / 8);
    FILE *f = fopen(k.filename, "rb");
    const size_t got = f ? fread(k.pos.data(), 8, k.pos.size(), f) : 0;
    if (f) fclose(f);
    if (got != k.pos.size()) {
        fprintf(stderr, "Invalid Parameters given: ZD_Glass_filename = %s cannot be read\n", k.filename);
        return 1;
    }
    for (size_t i = 0; i < k.pos.size(); i++)
        if (!(k.pos[i] >= 0.0 && k.pos[i] < 1.0)) {
            fprintf(stderr, "Invalid Parameters given: ZD_Glass_filename = %s: particle %llu = (%.17g, %.17g, %.17g) lies outside [0, 1)^3\n", k.filename,
                    (unsigned long long) (i / 3), k.pos[i / 3 * 3], k.pos[i / 3 * 3 + 1], k.pos[i / 3 * 3 + 2]);
            return 1;
        }
    return 0;
}

// one sweep of zd_displace into the output file: float64[9] per particle = position, displacement, velocity, in index order
struct GlassWriter {
    const GlassKeys *k = nullptr;
    FILE *f = nullptr;
    int64_t npart = 0, sweeps = 0;
    static int callback(void *user, int64_t first, int64_t n, const double *out6) {
        GlassWriter *w = (GlassWriter *) user;
        const int64_t t = w->k->tile;
        std::vector<double> row(9 * (size_t) std::min<int64_t>(n, 1 << 16));
        for (int64_t i0 = 0; i0 < n; i0 += 1 << 16) {
            const int64_t m = std::min<int64_t>(n - i0, 1 << 16);
            for (int64_t i = 0; i < m; i++) {
                const int64_t g = first + i0 + i, cell = g / w->npart, b = g % w->npart;
                const double off[3] = {(double) (cell % t), (double) ((cell / t) % t), (double) (cell / (t * t))};
                for (int j = 0; j < 3; j++) row[9 * i + j] = (w->k->pos[3 * b + j] + off[j]) / (double) t;
                memcpy(&row[9 * i + 3], out6 + 6 * (i0 + i), 6 * sizeof(double));
            }
            if (fwrite(row.data(), 72, (size_t) m, w->f) != (size_t) m) {
                fprintf(stderr, "Short write on the glass output file\n");
                return 1;
            }
        }
        w->sweeps++;
        return 0;
    }
};

// the run of a parameter file with ZD_Glass_filename: the planes feed the interpolation, no lattice file is written
static int glass_run(const GlassKeys &gk, const zd_params &p, const zd_param_strings &s, const zd_pk &pk, const double *eig, int64_t eig_ppd) {
    const fs::path out = gk.output[0] ? fs::path(gk.output) : fs::path(s.output_dir) / "ic_glass";
    GlassWriter w;
    w.k     = &gk;
    w.npart = (int64_t) gk.pos.size() / 3;
    w.f     = fopen(out.c_str(), "wb");
    if (!w.f) {
        fprintf(stderr, "Could not open output file \"%s\"\n", out.c_str());
        return 1;
    }
    zd_stats st;
    memset(&st, 0, sizeof(st));
    const int rc = zd_displace(&p, &pk, eig, eig_ppd, (int32_t) gk.order, w.npart, gk.pos.data(), gk.tile, 0, GlassWriter::callback, &w, &st);
    if (fclose(w.f) || rc) {
        fprintf(stderr, "zeldovich: the glass run failed\n");
        return 1;
    }
    fprintf(stderr, "glass: %lld particles, order %ld, %lld sweeps\n", (long long) (w.npart * gk.tile * gk.tile * gk.tile), gk.order, (long long) w.sweeps);
    fprintf(stderr, "Displacements at the particles took %f seconds (stream factor %d); written to %s\n", st.seconds_total, st.stream_factor, out.c_str());
    return 0;
}

// ZD_Field_filename, ZD_Field_kind (optional, not in the reference): the modes of the run come from a field instead of ZD_Seed
// (zd_generate_field); read with zd_param_file_string.  The file is a raw little-endian array [z][y][x]: 4 PPD^3 bytes = float32 (the
// layout of the density file a ZD_qdensity = 1 run writes), 8 PPD^3 bytes = float64.  It is mapped, not read: the library uploads it in
// chunks of planes.  ZD_Field_order (default 1; read only with ZD_Field_filename): 2 = second order on the field (zd_generate_field_lpt);
// ZD_q2LPT beside ZD_Field_filename keeps its refusal.
struct FieldKeys {
    char filename[1024] = "";
    int32_t kind = ZD_FIELD_DENSITY, dtype = ZD_FIELD_F32, order = 1;
    const void *data = nullptr;
};
static int read_field_keys(const char *path, FieldKeys &k) {
    char kind[1024];
    if (zd_param_file_string(path, "ZD_Field_filename", k.filename, sizeof(k.filename)) || zd_param_file_string(path, "ZD_Field_kind", kind, sizeof(kind)))
        return 1;
    if (!k.filename[0]) {
        if (kind[0]) {
            fprintf(stderr, "zeldovich_hip: ZD_Field_kind needs ZD_Field_filename (the field it describes)\n");
            return 1;
        }
        return 0;
    }
    if (kind[0] && strcmp(kind, "density") && strcmp(kind, "white")) {
        fprintf(stderr, "zeldovich_hip: ZD_Field_kind = %s must be \"density\" or \"white\"\n", kind);
        return 1;
    }
    k.kind = !strcmp(kind, "white") ? ZD_FIELD_WHITE : ZD_FIELD_DENSITY;
    char order[1024];
    if (zd_param_file_string(path, "ZD_Field_order", order, sizeof(order))) return 1;
    if (order[0]) {
        char *end = nullptr;
        const long n = strtol(order, &end, 10);
        if (*end || n < INT32_MIN || n > INT32_MAX) {
            fprintf(stderr, "zeldovich_hip: ZD_Field_order = %s must be an integer (1: Zel'dovich, 2: second order)\n", order);
            return 1;
        }
        k.order = (int32_t) n;  // (the library says which orders it runs)
    }
    return 0;
}
// the file against PPD, mapped; non-zero (one line) if it cannot be read or has neither size
static int map_field(FieldKeys &k, int64_t ppd) {
    const int fd = open(k.filename, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb)) {
        fprintf(stderr, "zeldovich_hip: ZD_Field_filename = %s cannot be read\n", k.filename);
        if (fd >= 0) close(fd);
        return 1;
    }
    const unsigned long long n3 = (unsigned long long) ppd * ppd * ppd, have = (unsigned long long) sb.st_size;
    if (have != 4 * n3 && have != 8 * n3) {
        fprintf(stderr, "zeldovich_hip: ZD_Field_filename = %s holds %llu bytes: a field of PPD = %lld is %llu bytes of float32 or %llu bytes of float64\n",
                k.filename, have, (long long) ppd, 4 * n3, 8 * n3);
        close(fd);
        return 1;
    }
    k.dtype = have == 8 * n3 ? ZD_FIELD_F64 : ZD_FIELD_F32;
    void *m = mmap(nullptr, (size_t) have, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) {
        fprintf(stderr, "zeldovich_hip: ZD_Field_filename = %s cannot be mapped\n", k.filename);
        return 1;
    }
    k.data = m;
    return 0;
}

int main(int argc, char *argv[]) {
    if (argc != 2) {
        fprintf(stderr, "Usage: %s param_file\n", argv[0]);
        exit(1);
    }
    const auto t_start = std::chrono::steady_clock::now();
    auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };

    LptKeys lk;  // (asked first: a refusal of these keys is the run's only line)
    if (read_lpt_keys(argv[1], lk)) exit(1);
    GlassKeys gk;
    if (read_glass_keys(argv[1], gk)) exit(1);
    FieldKeys fk;
    if (read_field_keys(argv[1], fk)) exit(1);
    zd_params p;
    zd_param_strings s;
    if (zd_params_from_file(argv[1], &p, &s)) {
        printf("Invalid Parameters given \n");
        exit(1);
    }
    zd_pk pk;
    zd_pk_handle *pkh = nullptr;
    if (s.Pk_filename[0]) {
        if (zd_pk_create_from_file(s.Pk_filename, s.Pk_scale, s.Pk_norm, s.Pk_sigma, s.Pk_sigma_ratio, s.Pk_smooth,
                                   s.qPk_fix_to_mean, p.boxsize, &pkh, &pk))
            return 1;
    } else {
        if (zd_pk_create_powerlaw(s.Pk_powerlaw_index, s.Pk_norm, s.Pk_sigma, s.Pk_sigma_ratio, s.Pk_smooth,
                                  s.qPk_fix_to_mean, p.boxsize, &pkh, &pk))
            return 1;
    }
    if (fk.filename[0]) {
        // (what reads the SEEDED modes of the parameters again — the self-checks, the band-power table — or runs its own passes)
        const char *other = gk.filename[0] ? "ZD_Glass_filename" : s.SelfCheck > 0 ? "ZD_SelfCheck" : s.Pk_measured_filename[0] ? "ZD_Pk_measured_filename"
                            : (lk.selfcheck > 0 || lk.pk_filename[0]) ? "ZD_LPT_SelfCheck / ZD_LPT_Pk_filename" : nullptr;
        if (other) {
            fprintf(stderr, "zeldovich_hip: ZD_Field_filename does not run together with %s on the command line (the plan calls of the library do)\n", other);
            exit(1);
        }
        if (map_field(fk, p.ppd)) exit(1);
        fprintf(stderr, "field: %s, %s, PPD %lld", fk.kind == ZD_FIELD_WHITE ? "white" : "density", fk.dtype == ZD_FIELD_F64 ? "float64" : "float32",
                (long long) p.ppd);
        if (fk.order != 1) fprintf(stderr, ", order %d", (int) fk.order);
        fprintf(stderr, "\n");
    }
    const int narray   = p.qdensity == 2 ? 1 : (p.qPLT ? 4 : 2);  // zeldovich.cpp:871-876
    const double memory = cube(p.ppd / 1024.0) * narray * 16.0;

    Writer w;
    w.p   = p;
    w.dir = s.output_dir;
    setup_output_dir(w.dir);
    static const int recsizes[4] = {32, 32, 56, 12};
    w.recsize     = p.qdensity == 2 ? 0 : recsizes[p.icformat];
    w.plane_bytes = (int64_t) p.ppd * p.ppd * w.recsize;
    if (const int nsites = s.SelfCheck > 0 ? s.SelfCheck : lk.selfcheck) {  // (never both)
        w.sites = self_check_sites(p, nsites);
        w.site_rec.assign((size_t) nsites * w.recsize, 0);
        w.site_dens.assign(nsites, 0.f);
        w.site_seen.assign(nsites, 0);
    }
    if (gk.filename[0] && (s.SelfCheck > 0 || lk.selfcheck > 0)) {
        fprintf(stderr, "Invalid Parameters given: ZD_Glass_filename does not run together with ZD_SelfCheck / ZD_LPT_SelfCheck: no lattice records are kept\n");
        exit(1);
    }
    if (p.qdensity && !gk.filename[0]) {  // InitOutputBuffers: output.cpp:282-288; "density{:d}" is an fmt pattern on ppd
        std::string name = s.density_filename;
        const size_t pos = name.find("{:d}");
        if (pos != std::string::npos) name.replace(pos, 4, std::to_string((long long) p.ppd));
        const fs::path path = w.dir / name;
        w.dens_fd           = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (w.dens_fd < 0) {
            fprintf(stderr, "Could not open density file \"%s\"\n", path.c_str());
            return 1;
        }
    }
    fprintf(stderr, "MI355X build: the whole problem (or one z-residue pass of it) resides in HBM.\n");
    fprintf(stderr, "Total array size: %5.3f GiB\n", memory);

    double *eig = nullptr;
    int64_t eig_ppd = 0;
    if (p.qPLT && s.PLT_compute_ppd) {  // the table computed on the GPU (ZD_PLT_compute_ppd) instead of loaded
        eig_ppd = s.PLT_compute_ppd;
        fprintf(stderr, "Computing PLT eigenmodes on %lld^3 points.\n", (long long) eig_ppd);
        eig = (double *) malloc((size_t) eig_ppd * eig_ppd * (eig_ppd / 2 + 1) * 4 * sizeof(double));  // (freed with zd_free, like a loaded one)
        if (!eig || zd_make_eigenmodes(eig_ppd, eig)) exit(1);
    } else if (p.qPLT && zd_load_eigmodes(s.PLT_filename, &eig, &eig_ppd))
        exit(1);
    char plt_write[1024];  // ZD_PLT_write_filename: the table this run uses, in the layout zd_load_eigmodes reads
    if (p.qPLT && (zd_param_file_string(argv[1], "ZD_PLT_write_filename", plt_write, sizeof(plt_write)) ||
                   (plt_write[0] && zd_write_eigmodes(plt_write, eig, eig_ppd))))
        exit(1);
    if (p.k_cutoff != 1)
        fprintf(stderr, "Using k_cutoff = %f (effective ppd = %d)\n", p.k_cutoff, (int) (p.ppd / p.k_cutoff + .5));
    fprintf(stderr, "Preamble took %f seconds\n", elapsed());

    if (gk.filename[0]) {  // an off-lattice load: the run's planes feed the interpolation
        if (glass_run(gk, p, s, pk, eig, eig_ppd)) exit(1);
        if (eig) zd_free(eig);
        zd_pk_destroy(pkh);
        fprintf(stderr, "zeldovich took %.4g sec for ppd %lld\n", elapsed(), (long long) p.ppd);
        return 0;
    }

    zd_stats st;
    memset(&st, 0, sizeof(st));
    if (fk.filename[0] && fk.order != 1 ? zd_generate_field_lpt(&p, &pk, fk.kind, fk.dtype, fk.data, 0, fk.order, Writer::callback, &w, &st)
        : fk.filename[0]                ? zd_generate_field(&p, &pk, eig, eig_ppd, fk.kind, fk.dtype, fk.data, 0, Writer::callback, &w, &st)
                                        : zd_generate(&p, &pk, eig, eig_ppd, Writer::callback, &w, &st)) {
        fprintf(stderr, "zeldovich: generation failed\n");
        exit(1);
    }
    fprintf(stderr, "Grid -> displacements took %f seconds on the GPU (stream factor %d, modes %s)\n", st.seconds_total,
            st.stream_factor, st.modes_cached ? "cached in HBM" : "generated per pass");
    fprintf(stderr, "Time so far: %f seconds\n", elapsed());

    // zeldovich.cpp:987-1011
    fprintf(stderr, "The rms density variation of the pixels is %f\n", sqrt(st.density_variance / cube((double) p.ppd)));
    fprintf(stderr, "This could be compared to the P(k) prediction of %f\n",
            zd_pk_sigmaR(&pk, (p.boxsize / p.ppd) / 4.0) * pow(p.boxsize, 1.5));
    if (p.qdensity != 2) {
        fprintf(stderr, "The maximum component-wise displacements are (%g, %g, %g), same units as BoxSize.\n",
                st.max_disp[0], st.max_disp[1], st.max_disp[2]);
        fprintf(stderr,
                "For Abacus' 2LPT implementation to work (assuming FINISH_WAIT_RADIUS = 1),\n\tthis implies a maximum CPD of %d\n",
                (int) (p.boxsize / (2 * fabs(st.max_disp[2]))));
    }
    if (s.Pk_measured_filename[0] && write_measured_power(s.Pk_measured_filename, p, pk, eig, eig_ppd)) exit(1);
    if (s.SelfCheck > 0 && self_check(w, s, pk, eig, eig_ppd)) exit(1);
    if (lk.pk_filename[0] && write_lpt_power(lk.pk_filename, p, pk)) exit(1);
    if (lk.selfcheck > 0 && lpt_self_check(w, lk, pk)) exit(1);
    w.close_all();
    fprintf(stderr, "WriteParticlesSlab took %.3g sec to write %.3g MB ==> %.3g MB/sec\n", w.seconds,
            w.bytes_written / 1e6, w.bytes_written / 1e6 / (w.seconds > 0 ? w.seconds : 1e-9));
    if (eig) zd_free(eig);
    zd_pk_destroy(pkh);
    const double tot = elapsed();
    fprintf(stderr, "zeldovich took %.4g sec for ppd %lld ==> %.3g Mpart/sec\n", tot, (long long) p.ppd,
            (double) s.np / 1e6 / tot);
    return 0;
}
