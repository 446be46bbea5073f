// Host build of phc_amd/csrc/phc_jpeg.h for tests/test_video_cpu.py, tests/test_video_gpu.py and tests/jpeg_asan_main.cpp: the argument check, the size
// functions, the code tables, and a whole launch of phc_jpeg_encode as loops over blocks, segments and frames (all pointers are host memory here).
#include "phc_jpeg.h"

extern "C" {

int jpeg_args_check_of(const phc_jpeg_args_t* a) { return phc::jpeg_args_check(a); }

int64_t jpeg_frame_bound_of(int w, int h, int ri) { return phc::jpeg_frame_bound(phc::jpeg_geom(w, h, ri)); }

int64_t jpeg_scratch_bytes_of(int64_t f, int w, int h, int ri) { return phc::jpeg_layout(phc::jpeg_geom(w, h, ri), f).total; }

int jpeg_block_max_bits() { return phc::JPEG_BLOCK_MAX_BITS; }

int jpeg_args_size() { return (int)sizeof(phc_jpeg_args_t); }

// out [2 * 12 + 2 * 256]: code << 5 | length of DC luminance, DC chrominance, AC luminance, AC chrominance
void jpeg_huff_table(uint32_t* out) {
    static const phc::JpegHuff h = phc::jpeg_huff_make();
    const uint32_t* p = reinterpret_cast<const uint32_t*>(&h);
    for (int i = 0; i < phc::JPEG_HUFF_WORDS; ++i) out[i] = p[i];
}

// phc_jpeg_encode's four launches on the host; -> what the entry point returns
int jpeg_encode_host(const phc_jpeg_args_t* a) {
    const int rc = phc::jpeg_args_check(a);
    if (rc) return rc;
    if (a->num_frames == 0) return 0;
    static const phc::JpegHuff h = phc::jpeg_huff_make();
    const phc::JpegK k = phc::jpeg_kargs(a);
    for (int64_t f = 0; f < k.F; ++f)
        for (int64_t b = 0; b < k.g.blocks; ++b) phc::jpeg_block(k, f, b);
    for (int64_t f = 0; f < k.F; ++f)
        for (int s = 0; s < k.g.nseg; ++s) phc::jpeg_segment(k, h, f, s);
    for (int64_t f = 0; f < k.F; ++f) {
        int32_t sum = 0;
        for (int s = 0; s < k.g.nseg; ++s) { k.seg_off[f * k.g.nseg + s] = sum; sum += k.seg_len[f * k.g.nseg + s]; }
        k.length[f] = sum;
    }
    for (int64_t fs = 0; fs < (int64_t)k.F * k.g.nseg; ++fs) phc::jpeg_copy_segment(k, fs, 0, 1);
    return 0;
}

}
