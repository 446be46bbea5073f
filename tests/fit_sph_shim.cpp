// Host build of phc_amd/csrc/phc_fit_sph.h for tests/test_fit_keypoints_cpu.py: phc_fit_sph_iterate's launches as loops over their tiles, frames and lanes
// (all pointers are host memory here), with the kernels' barriers as loop boundaries and the group's butterfly in its own order, and the argument checks.
#include <vector>
#include "phc_fit_sph.h"

using namespace phc;

extern "C" {

// the argument checks of phc_fit_sph_iterate, without the launches behind them
int fit_sph_args_check_of(const phc_fit_args_t* a, int iterations) { return check_fit_sph(a, iterations, nullptr); }

long long fit_sph_scratch_bytes_of(long long num_frames, int num_clips, int num_bodies) { return fit_sph_scratch_bytes(num_frames, num_clips, num_bodies); }

static void setup_host(const phc_fit_args_t& a, const FitScratch& s, int tf) {      // k_fit_setup
    int32_t run = 0;
    for (int c = 0; c < a.num_clips; ++c) {
        s.tile_start[c] = run;
        run += fit_clip_tiles(fit_span(a, c), tf);
        const FitCoef co = fit_coef(a.lr, a.step[c] + 1);
        s.coef[c * 2 + 0] = co.step_size; s.coef[c * 2 + 1] = co.bc2_sqrt;
    }
    s.tile_start[a.num_clips] = run;
}

static void frames_host(const phc_fit_args_t& a, const FitScratch& s, int64_t tiles) {
    const int G = 32, TF = FIT_BLOCK / G, NB = a.num_bodies;
    std::vector<float> s_pos(G * 3), s_L(G * 9), s_u(FIT_MAX_MATCHED * 3), R(G * 9), lanes(FIT_SUMS * G);
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const int c = fit_clip_of_tile(s.tile_start, a.num_clips, (int32_t)tile);
        if (c < 0) continue;
        const FitSpan sp = fit_span(a, c);
        const int64_t T = sp.t1 - sp.t0;
        float s_sum[8][FIT_SUMS];
        for (int fl = 0; fl < TF; ++fl) {
            const int64_t f = sp.t0 + ((tile - s.tile_start[c]) * TF + fl);
            const bool live = f >= sp.t0 && f < sp.t1;
            for (float& x : lanes) x = 0.f;
            if (live) {
                for (int b = 0; b < NB; ++b) fit_sph_local(a, f, b, &s_L[b * 9]);                           // stage A1
                for (int b = 0; b < NB; ++b) fit_sph_chain(a, f, c, b, s_L.data(), &s_pos[b * 3], &R[b * 9]);  // stage A2
                for (int m = 0; m < a.num_matched; ++m) {                                                   // stage B
                    float u[3], n;
                    fit_residual(a, f, m, s_pos.data(), u, &n);
                    for (int i = 0; i < 3; ++i) { s_u[m * 3 + i] = u[i]; lanes[i * G + m] = u[i]; }
                    lanes[3 * G + m] = n;
                }
                const FitCoef co = {s.coef[c * 2 + 0], s.coef[c * 2 + 1]};
                const float p0[3] = {s_pos[0], s_pos[1], s_pos[2]};
                fit_root_step(a, f, T, co, p0, s_pos.data(), s_u.data());                                   // stage C
                for (int j = 1; j < NB; ++j)
                    lanes[4 * G + j] = fit_sph_joint_step(a, f, j, T, co, &R[j * 9], s_L.data(), s_u.data(), s.clamped);
            }
            for (int i = 0; i < FIT_SUMS; ++i) s_sum[fl][i] = fit_group_sum_host(&lanes[i * G], G);
        }
        for (int i = 0; i < FIT_SUMS; ++i) {
            float acc = 0.f;
            for (int k = 0; k < TF; ++k) acc += s_sum[k][i];
            s.partial[tile * FIT_SUMS + i] = acc;
        }
    }
}

static void finish_host(const phc_fit_args_t& a, const FitScratch& s, const FitTaps& w, int64_t tiles) {
    const int ND = fit_sph_nd(a.num_bodies);
    for (int c = 0; c < a.num_clips; ++c) {
        const FitSpan sp = fit_span(a, c);
        for (int64_t t = sp.t0; t < sp.t1; ++t)
            for (int d = 0; d < ND; ++d) a.dof[t * ND + d] = fit_smooth(s.clamped, w, ND, d, t, sp.t0, sp.t1);
        for (int i = 0; i < 4; ++i) fit_sph_clip_lane(a, s, c, i, tiles);
        fit_clip_advance(a, s, c);
    }
}

// phc_fit_sph_iterate on the host
int fit_sph_iterate_host(const phc_fit_args_t* a, int iterations) {
    int64_t tiles = 0;
    const int rc = check_fit_sph(a, iterations, &tiles);
    if (rc) return rc;
    if (iterations == 0) return 0;
    const FitScratch s = fit_scratch(*a);
    const FitTaps w = fit_taps();
    setup_host(*a, s, fit_tile_frames(a->num_bodies));
    for (int it = 0; it < iterations; ++it) {
        frames_host(*a, s, tiles);
        finish_host(*a, s, w, tiles);
    }
    return 0;
}

}
