// A stand-alone run of the host build of phc_fit.h (tests/fit_shim.cpp) on the smallest batches, for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/fit_asan_main.cpp -o fit_asan && ./fit_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported.  A 3-body chain with one extended body
// (32-lane groups) and a 34-body chain (64-lane groups); clips of 1, 2 and 9 frames (a tile holds 8 or 4); 3 + 2 trips.  Run by tests/test_fit_device_cpu.py; CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fit_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

static int run(int NB, int E) {
    const int NBE = NB + E, ND = NB - 1, M = 2, C = 3;
    const int64_t start[C + 1] = {0, 1, 3, 12}, F = 12;
    int32_t* parents = heap<int32_t>(NBE, 0);
    for (int b = 0; b < NBE; ++b) parents[b] = b < NB ? b - 1 : 1;
    float* offsets = heap<float>(NBE * 3, 0.1f);
    for (int i = 0; i < NBE * 3; ++i) offsets[i] = 0.05f + 0.01f * (i % 7);
    float* rest = heap<float>(NBE * 9, 0.f);
    for (int b = 0; b < NBE; ++b) rest[b * 9] = rest[b * 9 + 4] = rest[b * 9 + 8] = 1.f;
    float* axis = heap<float>(ND * 3, 0.f);
    for (int j = 0; j < ND; ++j) axis[j * 3 + j % 3] = 1.f;
    float* range = heap<float>(ND * 2, 0.f);
    for (int j = 0; j < ND; ++j) { range[j * 2] = -0.01f; range[j * 2 + 1] = 1.f; }
    int32_t* match_body = heap<int32_t>(M, 0);
    match_body[1] = NBE - 1;                      // the root and the last (extended) body
    int32_t* match_slot = heap<int32_t>(M, 0);
    match_slot[1] = 1;
    uint32_t* subtree = heap<uint32_t>(NB, 0u);
    subtree[0] = 3u; subtree[1] = 2u;
    int64_t* clip_start = heap<int64_t>(C + 1, 0), *clip_start_host = heap<int64_t>(C + 1, 0);
    for (int c = 0; c <= C; ++c) clip_start[c] = clip_start_host[c] = start[c];
    float* target = heap<float>(F * M * 3, 0.3f);
    for (int i = 0; i < F * M * 3; ++i) target[i] = 0.3f + 0.02f * (i % 5);
    float* rto = heap<float>(F * 3, 0.2f);
    const int64_t sb = fit_scratch_bytes(F, C, NBE);
    phc_fit_args_t a = {};
    a.num_bodies = NB; a.num_ext = E; a.num_matched = M; a.num_clips = C; a.num_frames = F; a.lr = 0.02;
    a.parents = parents; a.offsets = offsets; a.rest = rest; a.axis = axis; a.range = range; a.match_body = match_body; a.match_slot = match_slot;
    a.subtree = subtree; a.clip_start = clip_start; a.clip_start_host = clip_start_host; a.target = target; a.root_trans_offset = rto;
    a.dof = heap<float>(F * ND, 0.f); a.dof_m = heap<float>(F * ND, 0.f); a.dof_v = heap<float>(F * ND, 0.f);
    a.root_rot = heap<float>(F * 3, 0.f); a.root_rot_m = heap<float>(F * 3, 0.f); a.root_rot_v = heap<float>(F * 3, 0.f);
    a.root_off = heap<float>(C * 3, 0.f); a.root_off_m = heap<float>(C * 3, 0.f); a.root_off_v = heap<float>(C * 3, 0.f);
    a.step = heap<int32_t>(C, 0); a.loss = heap<float>(C, 0.f);
    a.scratch = aligned_alloc(16, (size_t)sb); a.scratch_bytes = sb;
    int rc = fit_iterate_host(&a, 3);
    if (!rc) rc = fit_iterate_host(&a, 2);
    printf("NB %d E %d: rc %d, steps %d %d %d, loss %.6f %.6f %.6f, dof[0] %.6f\n", NB, E, rc, a.step[0], a.step[1], a.step[2], a.loss[0], a.loss[1], a.loss[2],
           a.dof[0]);
    const bool ok = rc == 0 && a.step[0] == 5 && a.step[2] == 5 && a.loss[0] == a.loss[0];
    void* all[] = {parents, offsets, rest, axis, range, match_body, match_slot, subtree, clip_start, clip_start_host, target, rto, a.dof, a.dof_m, a.dof_v,
                   a.root_rot, a.root_rot_m, a.root_rot_v, a.root_off, a.root_off_m, a.root_off_v, a.step, a.loss, a.scratch};
    for (void* p : all) free(p);
    return ok ? 0 : 1;
}

int main() {
    const int bad = run(3, 1) + run(34, 1);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
