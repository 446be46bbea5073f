// Host build of phc_amd/csrc/phc_clip.h for tests/test_clip_device_cpu.py: phc_clip_process's two launches as loops over their lanes (all pointers are
// host memory here), the filter's weights and the argument checks.
#include "phc_clip.h"

extern "C" {

// the argument checks of phc_clip_process, without the launches behind them
int clip_args_check_of(const phc_clip_args_t* a) { return phc::clip_args_check(a); }

long long clip_scratch_bytes_of(long long num_frames, int num_bodies) { return phc::clip_scratch_bytes(num_frames, num_bodies); }

int clip_frames_per_block_of(int num_bodies) { return phc::clip_frames_per_block(num_bodies); }

// out[17]: the weights of offsets -8 .. 8
void clip_weights(double* out) {
    const phc::ClipWeights w = phc::clip_gauss_weights();
    for (int i = 0; i <= phc::CLIP_RADIUS; ++i) out[i] = out[2 * phc::CLIP_RADIUS - i] = w.w[i];
}

// both kernels on the host: the same per-lane functions over all lanes, records written in place (the velocity columns by the second loop)
int clip_process_host(const phc_clip_args_t* a) {
    const int rc = phc::clip_args_check(a);
    if (rc) return rc;
    const int J = a->num_bodies;
    double* rows = (double*)a->scratch;
    int32_t* frame_clip = (int32_t*)(rows + a->num_frames * 6 * J);
    for (int64_t f = 0; f < a->num_frames; ++f) {
        const int c = phc::clip_of_frame(a->clip_start, a->num_clips, f);
        frame_clip[f] = c;
        float* rec = a->frames + f * a->frame_stride;
        for (int i = phc::clip_pad_begin(J); i < a->frame_stride; ++i) rec[i] = 0.f;
        for (int j = 0; j < J; ++j) {
            phc::ClipBody o;
            phc::clip_body(*a, f, j, phc::clip_span(*a, c, f), o);
            phc::clip_body_store(o, J, j, rec, rows + f * 6 * J);
        }
    }
    const phc::ClipWeights w = phc::clip_gauss_weights();
    for (int64_t f = 0; f < a->num_frames; ++f) {
        const phc::ClipSpan s = phc::clip_span(*a, frame_clip[f], f);
        for (int r = 0; r < 6 * J; ++r)
            a->frames[f * a->frame_stride + 7 * J + r] = (float)phc::clip_filtered_velocity(rows, w, J, r, f, s.t0, s.t1, s.dt);
    }
    return 0;
}

}
