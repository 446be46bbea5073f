// A stand-alone run of the host build of phc_record.h (tests/record_shim.cpp) for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/record_asan_main.cpp -o record_asan && ./record_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported.  motion_record_host over N in (1, 64, 65) x
// cap in (1, 2, 5) x both segment modes x with / without ref_body_pos and a per-env limit, cap + 3 calls each (a seed call first; the last calls overflow in
// every env), on a spherical model (24 bodies, 69 DoFs: the odd row width) and an all-revolute one with extended bodies (38 + 3 bodies: the 64-lane group).
// Not a pytest test of its own (tests/test_motion_record_cpu.py builds and runs it); CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "record_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

static int run(int N, int cap, int nb, int ne, bool revolute, int mode, bool with_limit) {
    const int nd = revolute ? nb - 1 : 3 * (nb - 1);
    // the model's tables, exactly as long as the kernel may read them: int tables 0 .. 20 of PHC_MAX_BODIES slots behind the 4 leading ints, PHC_BODY_FLOATS per slot
    int32_t* ints = heap<int32_t>(4 + 21 * PHC_MAX_BODIES, 0);
    float* floats = heap<float>((size_t)PHC_MAX_BODIES * PHC_BODY_FLOATS, 0.f);
    for (int j = 1; j < nb; ++j) {
        ints[4 + 2 * PHC_MAX_BODIES + j] = revolute ? PHC_JT_REVOLUTE : PHC_JT_SPHERICAL;
        ints[4 + 3 * PHC_MAX_BODIES + j] = revolute ? j - 1 : 3 * (j - 1);
        floats[j * PHC_BODY_FLOATS + 25 + j % 3] = 1.f;
    }
    phc_model_t m = {};
    m.num_bodies = nb; m.num_dof = nd; m.ints = ints; m.floats = floats; m.num_shapes = 1;
    phc_motion_record_args_t a = {};
    a.num_envs = N; a.num_bodies = nb; a.num_ext = ne; a.num_dof = nd; a.cap = cap; a.dt = 1.f / 30.f;
    a.flags = mode;
    a.width = record_width_of(nb, ne, nd, mode);
    float* root = heap<float>((size_t)N * 13, 0.25f);
    for (int i = 0; i < N; ++i) { float* q = root + i * 13 + 3; q[0] = 0.5f; q[1] = -0.5f; q[2] = 0.5f; q[3] = i % 2 ? 0.5f : -0.5f; }
    float* dof = heap<float>((size_t)N * nd * 2, 0.125f);
    float* rbs = heap<float>((size_t)N * nb * 13, 0.5f);
    int64_t* progress = heap<int64_t>(N, 3);
    int64_t* flag = heap<int64_t>(N, 0);
    int64_t* ids = heap<int64_t>(N, 11);
    float* t0 = heap<float>(N, 1.f);
    float* t1 = heap<float>(N, 0.5f);
    float* ref = (mode & PHC_RECORD_REF) ? heap<float>((size_t)N * nb * 3, 2.f) : nullptr;
    int32_t* limit = with_limit ? heap<int32_t>(N, 0) : nullptr;
    for (int i = 0; with_limit && i < N; ++i) limit[i] = i % (cap + 2);
    for (int i = 0; i < N; ++i) flag[i] = i % 3 == 0;
    float* frames = heap<float>((size_t)N * cap * a.width, -1.f);
    int32_t* header = heap<int32_t>((size_t)N * cap * 4, -1);
    int32_t *len = heap<int32_t>(N, 0), *seg = heap<int32_t>(N, 0), *closed = heap<int32_t>(N, 0), *dropped = heap<int32_t>(N, 0);
    a.root_states = root; a.dof_state = dof; a.rigid_body_state = rbs; a.progress_buf = progress; a.flag = flag; a.motion_ids = ids; a.motion_start_times = t0;
    a.motion_start_times_offset = t1; a.ref_body_pos = ref; a.limit = limit; a.frames = frames; a.header = header; a.len = len; a.seg = seg; a.closed = closed;
    a.dropped = dropped;
    int rc = 0;
    for (int c = 0; c < cap + 3 && !rc; ++c) {
        a.flags = mode | (c == 0 ? PHC_RECORD_SEED : 0);
        rc = motion_record_check_of(&m, &a);
        if (!rc) motion_record_host_of(&m, &a);
    }
    bool ok = rc == 0;
    for (int i = 0; i < N; ++i) {
        const int room = with_limit && limit[i] < cap ? limit[i] : cap;
        ok = ok && len[i] >= 0 && len[i] <= room && dropped[i] >= 0 && len[i] + dropped[i] <= cap + 3;
        if (!(mode & PHC_RECORD_ONE_SEGMENT)) ok = ok && len[i] == room && dropped[i] == cap + 3 - room && closed[i] == 0;
        for (int f = 0; f < cap; ++f)
            for (int c = 0; c < a.width; ++c) {
                const float v = frames[((size_t)i * cap + f) * a.width + c];
                ok = ok && std::isfinite(v) && (f < len[i] ? v != -1.f : v == -1.f);
            }
    }
    printf("N %d cap %d bodies %d + %d %s mode %d limit %d: rc %d, %s\n", N, cap, nb, ne, revolute ? "revolute" : "spherical", mode, (int)with_limit, rc, ok ? "ok" : "BAD");
    free(ints); free(floats); free(root); free(dof); free(rbs); free(progress); free(flag); free(ids); free(t0); free(t1); free(ref); free(limit); free(frames);
    free(header); free(len); free(seg); free(closed); free(dropped);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int N : {1, 64, 65})
        for (int cap : {1, 2, 5})
            for (int mode : {0, PHC_RECORD_ONE_SEGMENT, PHC_RECORD_REF, PHC_RECORD_REF | PHC_RECORD_ONE_SEGMENT})
                for (int lim = 0; lim < 2; ++lim) {
                    bad += run(N, cap, 24, 0, false, mode, lim != 0);
                    bad += run(N, cap, 38, 3, true, mode, lim != 0);
                }
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
