// A plain C++ restatement of the footprint albedo, DESIGN.md §4.24, written from the section's text; it includes no library header.
// Built by tests/footprint_ref.py with `g++ -O2 -ffp-contract=off`; tests/test_footprint_cpu.py holds it to the hand-derived answers
// of tests/footprint_cases.py, and the GPU tests hold the device to it bit for bit.
//
// §4.24 in short.  Factor f in 2..4, low-resolution frame w x h, full frame f·w x f·h, all arrays row-major.  For the
// low-resolution pixel q = (i, j) — column i, row j — with id = index_lo[q]:
//     n = 0;  s_ch = +0
//     for dy = 0 .. f-1 (outer), dx = 0 .. f-1 (inner):  p = (f·i + dx, f·j + dy)
//         if index_hi[p] == id:  n = n + 1;  if id >= 0:  s_ch = s_ch + albedo_hi[p, ch]
//     id < 0:   out_ch = 1       count = n
//     n == 0:   out = albedo_lo[q], its bits     count = 0
//     else:     out_ch = s_ch / f32(n)            count = n
#include <cstddef>
#include <cstdint>
#include <cstring>

extern "C" void footprint_mirror(const int32_t* index_lo, const float* albedo_lo, const int32_t* index_hi, const float* albedo_hi,
                                 uint32_t w, uint32_t h, uint32_t f, float* out, uint8_t* count_or_null) {
    const size_t W = (size_t)f * w;
    for (size_t j = 0; j < h; ++j) {
        for (size_t i = 0; i < w; ++i) {
            const size_t q = j * w + i;
            const int32_t id = index_lo[q];
            uint32_t n = 0;
            float s[3] = {0.0f, 0.0f, 0.0f};
            for (uint32_t dy = 0; dy < f; ++dy) {
                for (uint32_t dx = 0; dx < f; ++dx) {
                    const size_t p = (f * j + dy) * W + (f * i + dx);
                    if (index_hi[p] != id) continue;
                    n = n + 1;
                    if (id >= 0)
                        for (int ch = 0; ch < 3; ++ch) s[ch] = s[ch] + albedo_hi[3 * p + ch];
                }
            }
            if (id < 0) {
                for (int ch = 0; ch < 3; ++ch) out[3 * q + ch] = 1.0f;
            } else if (n == 0) {
                std::memcpy(out + 3 * q, albedo_lo + 3 * q, 3 * sizeof(float)); // the bits, a NaN's payload included
            } else {
                const float fn = (float)n;
                for (int ch = 0; ch < 3; ++ch) out[3 * q + ch] = s[ch] / fn;
            }
            if (count_or_null) count_or_null[q] = (uint8_t)n;
        }
    }
}
