// A stand-alone run of the host build of phc_proj.h (tests/proj_shim.cpp) for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/proj_asan_main.cpp -o proj_asan && ./proj_asan
// Every array is a heap allocation of exactly its stated size, so a read or write one element outside is reported.  N = 65 envs of a synthetic model (a grid
// of short capsules, the last two shapes extra capsules of the LAST body), the corner sizes: 24 bodies / 26 shapes and 62 bodies / 64 shapes, 1 and 4 slots,
// throws every 1 - 2 env steps from close by at the last body among others, resets through progress_buf and through the null pointer, 40 env steps each.
// Not a pytest test of its own (tests/test_projectile_cpu.py builds and runs it); CPU only.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "proj_shim.cpp"

template <class T> static T* heap(size_t n, T fill) {
    T* p = (T*)malloc(n * sizeof(T) + (n == 0));
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

static int run(int N, int NB, int P) {
    const int NS = NB + 2, STEPS = 40;
    phc_proj_args_t a = {};
    a.num_envs = N; a.num_bodies = NB; a.num_shapes = NS; a.num_listed = 3; a.count = P;
    a.pause_lo = 1; a.pause_hi = 2; a.life_steps = 6; a.substeps = 8;
    a.dt = 1.0f / 30; a.gravity_z = -9.81f; a.radius = 0.1f; a.restitution = 0.2f; a.friction = 1.0f;
    a.mass_lo = 1.f; a.mass_hi = 5.f; a.speed_lo = 5.f; a.speed_hi = 10.f; a.dist_lo = 0.5f; a.dist_hi = 1.0f; a.elev_lo = 0.f; a.elev_hi = 0.5f;
    a.key = 0x1234ABCD5678EF01ull; a.env_offset = ((int64_t)1 << 32) - N;                        // the last admissible offset
    int32_t* bodies = heap<int32_t>(3, 0);
    bodies[1] = NB / 2; bodies[2] = NB - 1;
    float* capsules = heap<float>((size_t)NS * 7, 0.f);
    int32_t* owner = heap<int32_t>(NS, NB - 1);
    for (int s = 0; s < NS; ++s) {
        if (s < NB) owner[s] = s;
        capsules[s * 7 + 0] = -0.1f; capsules[s * 7 + 3] = 0.1f; capsules[s * 7 + 6] = s % 7 == 3 ? 0.f : 0.05f;   // (some bodies have no shape)
        if (s >= NB) capsules[s * 7 + 2] = capsules[s * 7 + 5] = 0.1f * (s - NB + 1);
    }
    float* com = heap<float>((size_t)NB * 3, 0.01f), *inv_mass = heap<float>(NB, 0.5f), *inv_inertia = heap<float>((size_t)NB * 9, 0.f);
    for (int b = 0; b < NB; ++b) inv_inertia[b * 9 + 0] = inv_inertia[b * 9 + 4] = inv_inertia[b * 9 + 8] = 50.f;
    float* rbs = heap<float>((size_t)N * NB * 13, 0.f);
    for (int e = 0; e < N; ++e)
        for (int b = 0; b < NB; ++b) {
            float* r = rbs + ((size_t)e * NB + b) * 13;
            r[0] = 0.25f * (b % 8); r[1] = 0.25f * (b / 8); r[2] = 0.5f + 0.1f * (b % 3); r[6] = 1.f;
            r[7] = 0.1f * ((e + b) % 3 - 1); r[12] = 0.5f * ((e + 2 * b) % 3 - 1);
        }
    const size_t PN = (size_t)P * N;
    int32_t* life = heap<int32_t>(PN, 0), *countdown = heap<int32_t>(PN, 0), *thrown = heap<int32_t>(PN, 0), *hits = heap<int32_t>(PN, 0);
    int32_t* last_hit = heap<int32_t>(PN, -1), *k = heap<int32_t>(N, 0);
    float* pos = heap<float>(PN * 3, -1000.f), *vel = heap<float>(PN * 3, 0.f), *mass = heap<float>(PN, 0.f);
    float* force = heap<float>((size_t)N * NB * 3, 7.f), *torque = heap<float>((size_t)N * NB * 3, 7.f), *margin = heap<float>(N, 0.f);
    int64_t* progress = heap<int64_t>(N, 1);
    a.bodies = bodies; a.capsules = capsules; a.owner = owner; a.body_com = com; a.body_inv_mass = inv_mass; a.body_inv_inertia = inv_inertia;
    a.rigid_body_state = rbs; a.life = life; a.countdown = countdown; a.thrown = thrown; a.hits = hits; a.last_hit = last_hit; a.k = k; a.pos = pos; a.vel = vel;
    a.mass = mass; a.force = force; a.torque = torque;
    int rc = proj_args_check_of(&a);
    long long nthrown = 0, nhits = 0, last_body = 0, bad = 0;
    for (int t = 0; t < STEPS && !rc; ++t) {
        for (int e = 0; e < N; ++e) progress[e] = (e + t) % 11 == 0 ? 0 : t + 1;
        a.progress_buf = t % 5 == 4 ? nullptr : progress;
        proj_advance_host(&a, t % 2 ? margin : nullptr);
        for (size_t i = 0; i < (size_t)N * NB * 3; ++i) bad += !(force[i] == force[i]) || !(torque[i] == torque[i]);
        for (int e = 0; e < N; ++e) last_body += force[((size_t)e * NB + NB - 1) * 3] != 0.f || force[((size_t)e * NB + NB - 1) * 3 + 2] != 0.f;
    }
    for (size_t i = 0; i < PN; ++i) { nthrown += thrown[i]; nhits += hits[i]; }
    int kk = 1;
    for (int e = 0; e < N; ++e) kk &= k[e] == STEPS;
    printf("N %d NB %d P %d: rc %d, thrown %lld, hits %lld, steps with a force on the last body %lld, NaN %lld, k ok %d\n", N, NB, P, rc, nthrown, nhits, last_body, bad, kk);
    const bool ok = rc == 0 && nthrown > N && nhits > N / 2 && last_body > 0 && bad == 0 && kk;
    void* all[] = {bodies, capsules, owner, com, inv_mass, inv_inertia, rbs, life, countdown, thrown, hits, last_hit, k, pos, vel, mass, force, torque, margin, progress};
    for (void* p : all) free(p);
    return ok ? 0 : 1;
}

int main() {
    int fails = 0;
    for (int nb : {24, 62})
        for (int p : {1, 4}) fails += run(65, nb, p);
    fails += run(1, 24, 4);
    if (fails) { printf("proj_asan: %d case(s) failed\n", fails); return 1; }
    printf("proj_asan: ok\n");
    return 0;
}
