// A stand-alone run of the host build of phc_jpeg.h (tests/jpeg_shim.cpp) for the host sanitizers:
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -ffp-contract=off -std=c++17 -I phc_amd/csrc tests/jpeg_asan_main.cpp -o jpeg_asan && ./jpeg_asan
// Every array is a heap allocation of exactly its stated size (the output of exactly phc_jpeg_frame_bound per frame, the scratch of exactly
// phc_jpeg_scratch_bytes), so a read or write one byte outside is reported.  The inputs are the ones that code longest: uniform noise and saturated alternating
// pixels under all-ones quantiser tables (every coefficient survives), at sizes with both edges extended, restart intervals 1, 3 and one past the frame, one
// and three frames, padded rows.  Not a pytest test of its own (tests/test_video_cpu.py builds and runs it); CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "jpeg_shim.cpp"

static int run(int F, int W, int H, int ri, int pattern, int row_pad, bool with_coef) {
    phc_jpeg_args_t a = {};
    a.num_frames = F; a.width = W; a.height = H; a.restart_interval = ri;
    a.row_stride = 4 * (int64_t)W + row_pad; a.frame_stride = a.row_stride * H;
    uint8_t* rgba = (uint8_t*)malloc((size_t)(a.frame_stride * F));
    uint32_t s = 12345u + (uint32_t)pattern;
    for (int64_t i = 0; i < a.frame_stride * F; ++i) {
        s = s * 1664525u + 1013904223u;
        const int64_t x = (i % a.row_stride) / 4, y = (i / a.row_stride) % H;
        rgba[i] = pattern == 0 ? (uint8_t)(s >> 24) : (((x + y) & 1) ? 255 : 0);
    }
    uint8_t qtab[128];
    memset(qtab, 1, sizeof qtab);
    const int64_t bound = jpeg_frame_bound_of(W, H, ri), need = jpeg_scratch_bytes_of(F, W, H, ri);
    const int64_t blocks = 6 * (int64_t)((W + 15) / 16) * ((H + 15) / 16);
    uint8_t* out = (uint8_t*)malloc((size_t)(bound * F));
    int32_t* length = (int32_t*)malloc(sizeof(int32_t) * F);
    void* coef = nullptr;
    void* scratch = nullptr;
    if (with_coef && posix_memalign(&coef, 16, (size_t)(F * blocks * 128))) return 1;
    if (posix_memalign(&scratch, 16, (size_t)need)) return 1;
    a.rgba = rgba; a.qtab = qtab; a.out = out; a.out_stride = bound; a.length = length; a.coef = (int16_t*)coef; a.scratch = scratch; a.scratch_bytes = need;
    const int rc = jpeg_encode_host(&a);
    long long total = 0, worst = 0;
    for (int f = 0; f < F && !rc; ++f) { total += length[f]; worst = length[f] > worst ? length[f] : worst; }
    printf("F %d %dx%d ri %d pattern %d: rc %d, %lld bytes, largest frame %lld of bound %lld\n", F, W, H, ri, pattern, rc, total, worst, (long long)bound);
    const bool ok = rc == 0 && total > 0 && worst <= bound;
    free(rgba); free(out); free(length); free(coef); free(scratch);
    return ok ? 0 : 1;
}

int main() {
    int fails = 0;
    for (int pattern : {0, 1})
        for (int ri : {1, 3, 1000}) {
            fails += run(1, 17, 9, ri, pattern, 0, true);
            fails += run(3, 40, 33, ri, pattern, 12, false);
        }
    if (fails) { printf("jpeg_asan: %d case(s) failed\n", fails); return 1; }
    printf("jpeg_asan: ok\n");
    return 0;
}
