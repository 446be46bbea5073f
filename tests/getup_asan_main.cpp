// A stand-alone run of the host build of phc_getup.h (tests/getup_shim.cpp) for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/getup_asan_main.cpp -o getup_asan && ./getup_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported.  Two cases at N = 65 and N = 1025 (one past the
// wavefront and one past the scan tile), D = 3: the tight pool (every env holds a slot, every other env is done and falls: F == n_f) and done envs whose
// `assign` lies outside [0, N) (they release nothing).  Not a pytest test of its own (tests/test_getup_device_cpu.py builds and runs it); CPU only.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "getup_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

static int run(int N, bool tight) {
    const int D = 3;
    float* prob = heap<float>(2, 0.f);
    prob[1] = 1.f;                                             // every done env falls
    int64_t* reset_buf = heap<int64_t>(N, 0), *terminate_buf = heap<int64_t>(N, 1), *avail = heap<int64_t>(N, tight ? 1 : 0), *assign = heap<int64_t>(N, 0);
    int n_done = 0;
    for (int i = 0; i < N; ++i) {
        reset_buf[i] = i % 2 == 0;
        n_done += i % 2 == 0;
        if (tight) assign[i] = ((int64_t)i * 7 + 3) % N;                                  // N = 65, 1025 are coprime to 7: a bijection
        else assign[i] = i % 4 == 0 ? N : (i % 4 == 2 ? -1 : ((int64_t)1 << 40));         // outside [0, N) either way
    }
    float* fall_root = heap<float>((size_t)N * 13, 0.5f), *fall_dof_pos = heap<float>((size_t)N * D, 0.25f);
    float* root_states = heap<float>((size_t)N * 13, 0.f), *dof_state = heap<float>((size_t)N * D * 2, 1.f);
    int32_t* recovery_counter = heap<int32_t>(N, 0), *k = heap<int32_t>(N, 0), *kind = heap<int32_t>(N, 9), *free_list = heap<int32_t>(N, -7);
    int64_t* launch_count = heap<int64_t>(1, 5), *normal_flag = heap<int64_t>(N, 9), *fall_list = heap<int64_t>(N, -7);
    phc_getup_args_t a = {};
    a.num_envs = N; a.num_dof = D; a.recovery_steps = 8; a.key = 0x1234ABCD5678EF01ull; a.env_offset = 0;
    a.prob = prob; a.reset_buf = reset_buf; a.terminate_buf = terminate_buf; a.fall_root = fall_root; a.fall_dof_pos = fall_dof_pos; a.root_states = root_states;
    a.dof_state = dof_state; a.avail = avail; a.assign = assign; a.recovery_counter = recovery_counter; a.k = k; a.launch_count = launch_count; a.kind = kind;
    a.normal_flag = normal_flag; a.fall_list = fall_list; a.free_list = free_list;
    int rc = getup_args_check_of(&a);
    if (!rc) getup_assign_host_of(&a, nullptr, nullptr);
    int held = 0, falls = 0, moved = 0;
    for (int i = 0; i < N; ++i) {
        held += avail[i] != 0;
        falls += kind[i] == 3;
        moved += kind[i] == 3 && root_states[(size_t)i * 13] == 0.5f && dof_state[(size_t)i * D * 2 + 1] == 0.f && recovery_counter[i] == 8;
    }
    printf("N %d %s: rc %d, done %d, FALL %d, teleported %d, slots held %d, launch count %lld\n", N, tight ? "tight pool" : "assign out of range", rc, n_done, falls,
           moved, held, (long long)*launch_count);
    // tight: the released slots are exactly the ones taken again (the pool stays full); out of range: nothing was released, the fallers took n_done fresh slots
    const bool ok = rc == 0 && falls == n_done && moved == n_done && held == (tight ? N : n_done) && *launch_count == 6;
    void* all[] = {prob, reset_buf, terminate_buf, avail, assign, fall_root, fall_dof_pos, root_states, dof_state, recovery_counter, k, kind, free_list, launch_count,
                   normal_flag, fall_list};
    for (void* p : all) free(p);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    for (int N : {65, 1025})
        for (bool tight : {true, false}) bad += run(N, tight);
    // phc_task_draws: both outputs, then each alone
    const int N = 65;
    int32_t* k = heap<int32_t>(N, 0);
    float* phase = heap<float>(N, -1.f), *off = heap<float>((size_t)N * 2, -1.f);
    task_draws_host(N, 7ull, 0, k, phase, off);
    task_draws_host(N, 7ull, 0, k, nullptr, off);
    task_draws_host(N, 7ull, 0, k, phase, nullptr);
    bad += !(k[N - 1] == 3 && phase[N - 1] >= 0.f && phase[N - 1] < 1.f && off[2 * N - 1] >= 0.f && off[2 * N - 1] < 1.f);
    free(k); free(phase); free(off);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
