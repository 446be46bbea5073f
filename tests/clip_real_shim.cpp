// Host build of phc_amd/csrc/phc_clip_real.h for tests/test_clip_real_cpu.py: phc_clip_process_real's three launches as loops over their lanes (all pointers
// are host memory here) and the argument checks.
#include "phc_clip_real.h"

extern "C" {

// the argument checks of phc_clip_process_real, without the launches behind them
int clip_real_args_check_of(const phc_clip_real_args_t* a) { return phc::clip_real_args_check(a); }

long long clip_real_scratch_bytes_of(long long num_frames, int num_bodies, int num_clips) { return phc::clip_real_scratch_bytes(num_frames, num_bodies, num_clips); }

int clip_real_frames_per_block_of(int num_bodies, int num_ext) { return phc::clip_real_frames_per_block(num_bodies, num_ext); }

int clip_real_stride_of(int num_bodies, int num_ext) { return phc::clip_real_stride(num_bodies, num_ext); }

// the three kernels on the host: the same per-lane functions over all lanes, records written in place (the velocity columns by the last loop)
int clip_real_process_host(const phc_clip_real_args_t* a) {
    const int rc = phc::clip_real_args_check(a);
    if (rc) return rc;
    const int NB = a->num_bodies, E = a->num_ext, J = NB + E;
    double* rows = (double*)a->scratch;
    double* dz = phc::clip_real_dz(*a);
    int32_t* frame_clip = phc::clip_real_frame_clip(*a);
    for (int c = 0; c < a->num_clips; ++c) {
        dz[c] = 0.0;
        if (!a->fix_height) continue;
        double body4[phc::CLIP_MAX_BODIES * 4];
        const int64_t f0 = phc::clip_real_first_frame(*a, c);
        for (int j = 0; j < NB; ++j) phc::clip_real_height_body(*a, f0, j, body4 + 4 * j);
        double z = INFINITY;
        for (int k = 0; k < a->num_contacts; ++k) z = fmin(z, phc::clip_real_contact_z(*a, body4, k));
        dz[c] = z;
    }
    for (int64_t f = 0; f < a->num_frames; ++f) {
        const int c = phc::clip_of_frame(a->clip_start, a->num_clips, f);
        frame_clip[f] = c;
        float* rec = a->frames + f * a->frame_stride;
        for (int i = phc::clip_real_pad_begin(NB, E); i < a->frame_stride; ++i) rec[i] = 0.f;
        for (int j = 0; j < J; ++j) {
            phc::ClipRealBody o;
            phc::clip_real_body(*a, f, j, phc::clip_real_span(*a, c, f), o);
            phc::clip_real_body_store(o, NB, E, j, rec, rows + f * 6 * NB);
        }
    }
    const phc::ClipWeights w = phc::clip_gauss_weights();
    for (int64_t f = 0; f < a->num_frames; ++f) {
        const phc::ClipRealSpan s = phc::clip_real_span(*a, frame_clip[f], f);
        for (int r = 0; r < 6 * NB; ++r)
            a->frames[f * a->frame_stride + 7 * J + r] = (float)phc::clip_filtered_velocity(rows, w, NB, r, f, s.t0, s.t1, s.dt);
    }
    return 0;
}

}
