// A stand-alone run of the host build of phc_obs_aug.h (tests/obs_aug_shim.cpp) for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/obs_aug_asan_main.cpp -o obs_aug_asan && ./obs_aug_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported.  obs_augment_host over the shapes of
// tests/obs_aug_util.py's CASES in all three selection forms (every row, every other row flagged, the odd rows listed backwards plus an id outside [0, N)), and
// occl_advance_host over N in (1, 65, 257) x J in (1, 9, 24, 25, 64).  Not a pytest test of its own (tests/test_obs_aug_cpu.py builds and runs it); CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "obs_aug_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

struct Case { int N, num_obs, so, T; float p, std; };

static int run(const Case& c, int form) {
    float* obs = heap<float>((size_t)c.N * c.num_obs, 1.f);
    int32_t* k = heap<int32_t>(c.N, 3);
    int64_t* flag = heap<int64_t>(c.N, 0);
    const int n_ids = c.N / 2 + 1;                       // the odd rows backwards, then one id outside [0, N)
    int64_t* ids = heap<int64_t>(n_ids, (int64_t)c.N);
    int selected = 0;
    for (int i = 0; i < c.N; ++i) flag[i] = i % 2 == 0 ? 2 : 0;
    for (int r = 0, i = c.N - 1 - c.N % 2; r < n_ids - 1; ++r, i -= 2) ids[r] = i;   // N / 2 odd rows
    phc_obs_aug_args_t a = {};
    a.num_envs = c.N; a.num_obs = c.num_obs; a.self_obs_size = c.so; a.num_samples = c.T; a.dropout_p = c.p; a.noise_std = c.std;
    a.key = 0x0F1E2D3C4B5A6978ull; a.env_offset = 5; a.obs = obs; a.k = k;
    if (form == 1) a.row_flag = flag;
    if (form == 2) { a.env_ids = ids; a.n_ids = n_ids; }
    const int rc = obs_augment_check_of(&a);
    if (!rc) obs_augment_host_of(&a);
    bool ok = rc == 0;
    for (int i = 0; i < c.N; ++i) {
        const bool sel = form == 0 || (form == 1 ? i % 2 == 0 : i % 2 == 1);
        selected += sel;
        ok = ok && k[i] == (sel ? 4 : 3);
        for (int col = 0; col < c.num_obs; ++col) {
            const float v = obs[(size_t)i * c.num_obs + col];
            ok = ok && std::isfinite(v) && (sel || v == 1.f) && std::fabs(v - 1.f) <= 1.f + 0.1f * 5.77f;
        }
    }
    printf("N %d num_obs %d so %d T %d p %g std %g form %d: rc %d, selected %d, %s\n", c.N, c.num_obs, c.so, c.T, c.p, c.std, form, rc, selected, ok ? "ok" : "BAD");
    free(obs); free(k); free(flag); free(ids);
    return ok ? 0 : 1;
}

static int run_occl(int N, int J) {
    int32_t* k = heap<int32_t>(N, 0);
    int64_t* count = heap<int64_t>((size_t)N * J, 2);
    uint8_t* mask = heap<uint8_t>((size_t)N * J, 7);
    int rc = 0;
    for (int step = 0; step < 3 && !rc; ++step) {
        rc = occl_advance_check_of(N, J, 0, k, 0.1f, 30, 60, count, mask);
        if (!rc) occl_advance_host_of(N, J, 0x8796A5B4C3D2E1F0ull, 0, k, 0.1f, 30, 60, count, mask);
    }
    bool ok = rc == 0;
    for (int i = 0; i < N; ++i) {
        ok = ok && k[i] == 3;
        for (int j = 0; j < J; ++j)
            ok = ok && count[(size_t)i * J + j] >= 0 && count[(size_t)i * J + j] <= 58 && mask[(size_t)i * J + j] == !(9 <= j && j < 24) && (j != 0 || count[(size_t)i * J] == 0);
    }
    free(k); free(count); free(mask);
    return ok ? 0 : 1;
}

int main() {
    const Case cases[] = {{1, 1, 0, 1, 0.f, 0.1f}, {2, 2, 1, 1, 0.1f, 0.1f}, {63, 7, 1, 3, 0.1f, 0.1f}, {64, 255, 0, 3, 1.f, 0.1f}, {65, 256, 1, 3, 0.1f, 0.1f},
                          {257, 257, 257, 1, 0.1f, 0.1f}, {2, 513, 0, 3, 0.1f, 0.f}, {65, 1025, 1, 1, 0.f, 0.1f}, {63, 1025, 1025, 3, 1.f, 0.1f}, {257, 7, 1, 3, 1.f, 0.f},
                          {64, 513, 0, 3, 0.1f, 0.1f}, {1, 257, 1, 1, 0.1f, 0.1f}, {2, 255, 0, 3, 0.1f, 0.1f}, {65, 2, 0, 1, 0.f, 0.f}, {64, 256, 1, 3, 0.f, 0.1f},
                          {257, 1, 1, 3, 0.1f, 0.1f}};
    int bad = 0;
    for (const Case& c : cases)
        for (int form = 0; form < 3; ++form) bad += run(c, form);
    for (int N : {1, 65, 257})
        for (int J : {1, 9, 24, 25, 64}) bad += run_occl(N, J);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
