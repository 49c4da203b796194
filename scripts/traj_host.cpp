// scripts/traj_host.cpp — the CPU yardstick of scripts/traj_timing.py: the rule of limo-velo_amd/csrc/lv_traj.hpp (the very functions
// the kernels run) on one core, over files of raw little-endian arrays.  Not part of the library.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -Itests/emu -Ilimo-velo_amd/csrc scripts/traj_host.cpp -o scripts/traj_host
//   traj_host register knots.bin xyz.bin times.bin out.bin   knots: n x lv_traj_knot; xyz: m x 3 f32; times: m f64 -> out: m x 3 f32
//   traj_host smooth knots.bin sigma half_window iterations out.bin                                    -> out: n x lv_traj_knot
// Registration: world frame, identity extrinsic, LV_TRAJ_CLAMP, every point by its own search of the whole time array.  Prints the
// milliseconds of the loop alone (files and the interval records excluded) as one JSON line.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "lv_traj.hpp"

emu_dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace lv {
void set_error(const char*, ...) {}
}  // namespace lv

using namespace lv;

template <class T>
static std::vector<T> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
template <class T>
static void dump(const char* path, const std::vector<T>& v) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "register" && argc == 6) {
        const auto knots = slurp<lv_traj_knot>(argv[2]);
        const auto xyz = slurp<float>(argv[3]);
        const auto at = slurp<double>(argv[4]);
        const uint32_t n = (uint32_t)knots.size();
        const size_t m = at.size();
        std::vector<TrajDerived> der(n, TrajDerived{});
        std::vector<double> times(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (i + 1 < n) traj_derive(knots[i], knots[i + 1], &der[i]);
            times[i] = knots[i].time;
        }
        lv_traj_register_params prm;
        default_traj_register_params(&prm);
        double E[12];
        traj_rigid(prm.ext_t, prm.ext_q, E);
        std::vector<float> out(3 * m);
        const double t0 = now_ms();
        for (size_t k = 0; k < m; ++k) {
            lv_graph_pose T;
            const int st = traj_pose_at(times.data(), knots.data(), der.data(), 0, n, n, at[k], LV_TRAJ_CLAMP, &T);
            traj_register_point(E, T, st, nullptr, &xyz[3 * k], &out[3 * k]);
        }
        const double ms = now_ms() - t0;
        dump(argv[5], out);
        printf("{\"mode\": \"register\", \"knots\": %u, \"points\": %zu, \"ms\": %.3f}\n", n, m, ms);
    } else if (mode == "smooth" && argc == 7) {
        auto knots = slurp<lv_traj_knot>(argv[2]);
        const double sigma = atof(argv[3]);
        const uint32_t hw = (uint32_t)atoi(argv[4]);
        const int iters = atoi(argv[5]);
        const uint32_t n = (uint32_t)knots.size();
        std::vector<lv_traj_knot> next(n);
        const double t0 = now_ms();
        for (int it = 0; it < iters; ++it) {   // pin_ends = 1, nothing else fixed
            for (uint32_t i = 0; i < n; ++i) {
                if (i == 0 || i + 1 == n) next[i] = knots[i];
                else traj_smooth_knot(knots.data(), n, i, sigma, hw, &next[i]);
            }
            knots.swap(next);
        }
        const double ms = now_ms() - t0;
        dump(argv[6], knots);
        printf("{\"mode\": \"smooth\", \"knots\": %u, \"iterations\": %d, \"ms\": %.3f}\n", n, iters, ms);
    } else {
        fprintf(stderr, "usage: traj_host register knots xyz times out | traj_host smooth knots sigma half_window iterations out\n");
        return 2;
    }
    return 0;
}
