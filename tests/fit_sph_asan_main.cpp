// A stand-alone run of the host build of phc_fit_sph.h (tests/fit_sph_shim.cpp) on the smallest batches, for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/fit_sph_asan_main.cpp -o fit_sph_asan && ./fit_sph_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported; `axis` is null.  A 4-body tree (a chain
// with a branch), a 1-body model (no joints) and a 32-body chain (every lane of the group, the longest ancestor mask); clips of 1, 2 and 9 frames (a tile
// holds 8); 3 + 2 trips.  Run by tests/test_fit_keypoints_cpu.py; CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fit_sph_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

static int run(int NB, bool branch) {
    const int ND = 3 * (NB - 1), M = NB > 1 ? 2 : 1, C = 3;
    const int64_t start[C + 1] = {0, 1, 3, 12}, F = 12;
    int32_t* parents = heap<int32_t>(NB, 0);
    for (int b = 0; b < NB; ++b) parents[b] = b - 1;
    if (branch) parents[NB - 1] = 1;
    float* offsets = heap<float>(NB * 3, 0.1f);
    for (int i = 0; i < NB * 3; ++i) offsets[i] = 0.05f + 0.01f * (i % 7);
    float* rest = heap<float>(NB * 9, 0.f);
    for (int b = 0; b < NB; ++b) rest[b * 9] = rest[b * 9 + 4] = rest[b * 9 + 8] = 1.f;
    float* range = heap<float>(ND * 2, 0.f);
    for (int j = 0; j < ND; ++j) { range[j * 2] = -0.01f; range[j * 2 + 1] = 1.f; }
    int32_t* match_body = heap<int32_t>(M, 0);
    int32_t* match_slot = heap<int32_t>(M, 0);
    uint32_t* subtree = heap<uint32_t>(NB, 0u);
    subtree[0] = M == 2 ? 3u : 1u;
    if (M == 2) {                                 // the root and the last body
        match_body[1] = NB - 1; match_slot[1] = 1;
        for (int k = NB - 1; k > 0; k = parents[k]) subtree[k] = 2u;
    }
    int64_t* clip_start = heap<int64_t>(C + 1, 0), *clip_start_host = heap<int64_t>(C + 1, 0);
    for (int c = 0; c <= C; ++c) clip_start[c] = clip_start_host[c] = start[c];
    float* target = heap<float>(F * M * 3, 0.3f);
    for (int i = 0; i < F * M * 3; ++i) target[i] = 0.3f + 0.02f * (i % 5);
    float* rto = heap<float>(F * 3, 0.2f);
    const int64_t sb = fit_sph_scratch_bytes(F, C, NB);
    phc_fit_args_t a = {};
    a.num_bodies = NB; a.num_ext = 0; a.num_matched = M; a.num_clips = C; a.num_frames = F; a.lr = 0.02;
    a.parents = parents; a.offsets = offsets; a.rest = rest; a.axis = nullptr; a.range = range; a.match_body = match_body; a.match_slot = match_slot;
    a.subtree = subtree; a.clip_start = clip_start; a.clip_start_host = clip_start_host; a.target = target; a.root_trans_offset = rto;
    a.dof = heap<float>(F * ND, 0.f); a.dof_m = heap<float>(F * ND, 0.f); a.dof_v = heap<float>(F * ND, 0.f);
    a.root_rot = heap<float>(F * 3, 0.f); a.root_rot_m = heap<float>(F * 3, 0.f); a.root_rot_v = heap<float>(F * 3, 0.f);
    a.root_off = heap<float>(C * 3, 0.f); a.root_off_m = heap<float>(C * 3, 0.f); a.root_off_v = heap<float>(C * 3, 0.f);
    a.step = heap<int32_t>(C, 0); a.loss = heap<float>(C, 0.f);
    a.scratch = aligned_alloc(16, (size_t)sb); a.scratch_bytes = sb;
    int rc = fit_sph_iterate_host(&a, 3);
    if (!rc) rc = fit_sph_iterate_host(&a, 2);
    printf("NB %d: rc %d, steps %d %d %d, loss %.6f %.6f %.6f, root_rot[0] %.6f\n", NB, rc, a.step[0], a.step[1], a.step[2], a.loss[0], a.loss[1], a.loss[2],
           a.root_rot[0]);
    const bool ok = rc == 0 && a.step[0] == 5 && a.step[2] == 5 && a.loss[0] == a.loss[0];
    void* all[] = {parents, offsets, rest, range, match_body, match_slot, subtree, clip_start, clip_start_host, target, rto, a.dof, a.dof_m, a.dof_v,
                   a.root_rot, a.root_rot_m, a.root_rot_v, a.root_off, a.root_off_m, a.root_off_v, a.step, a.loss, a.scratch};
    for (void* p : all) free(p);
    return ok ? 0 : 1;
}

int main() {
    const int bad = run(4, true) + run(1, false) + run(32, false);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
