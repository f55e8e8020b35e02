// vggish.h -- launch functions of the VGGish feature path (vggish.hip): data/usc/features.py:166-240 with vggish/mel_features.py,
// vggish_input.py, vggish_slim.py and vggish_postprocess.py.  Every launch goes to the given stream and never syncs; every result
// is deterministic (no float atomics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace l3 {

constexpr int VG_SR = 16000;                 // vggish_input.py:25 target_sample_rate
constexpr int VG_WIN = 400, VG_HOP = 160;    // 25 ms / 10 ms at 16 kHz (vggish_input.py:26-27)
constexpr int VG_NFFT = 512, VG_BINS = 257;  // mel_features.py:209
constexpr int VG_MELS = 64;                  // vggish_input.py:27 num_mel_bins
constexpr int VG_ROWS = 96;                  // frame_win_sec 0.96 at 100 log-mel rows per second
constexpr int VG_EMB = 128;
constexpr int VG_LM_FRAMES = 32;             // frames per log-mel workgroup (one MFMA tile of rows)
constexpr int VG_BIN_BLOCKS = 9;             // 32-bin blocks of the spectrum: 288 >= 257
constexpr int VG_BINS_PAD = VG_BIN_BLOCKS * 32;
constexpr int VG_DFT_COLS = VG_BIN_BLOCKS * 64;      // per block: 32 real columns, then the 32 imaginary ones

void vggish_host_dft(std::vector<float>* dft);       // [VG_WIN][VG_DFT_COLS]: periodic Hann x DFT basis
void vggish_host_mel(std::vector<float>* mel);       // [VG_BINS_PAD][VG_MELS]
// segments {offset, length} of a 16 kHz buffer -> blocks {first sample, frames (1..32), first output row} and, if asked, each
// segment's first log-mel row (+ the total at the end); returns the number of log-mel rows (1 + (len - 400) / 160 per segment)
int64_t vggish_logmel_blocks(const int64_t* segs, int64_t n_seg, std::vector<int64_t>* blocks, std::vector<int64_t>* seg_row0);
// out (rows, 64) = log(|rfft(frame x hann, 512)| . mel + 0.01), one workgroup per block
void vggish_logmel(const float* x, const int64_t* blocks, int64_t n_blocks, const float* dft, const float* mel, float* out,
                   hipStream_t s);
// y (n, 48, 32, 64) = maxpool2(relu(conv3x3_same(example e) + b)), example e = log-mel rows [ex_rows[e], + 96); w (3, 3, 1, 64)
void vggish_conv1(const float* logmel, const int64_t* ex_rows, const float* w, const float* b, float* y, int n, hipStream_t s);
// y = relu(x + b) (pool 0; in place allowed) or its 2x2 / stride-2 maximum (pool 1; H, W even); x (n, H, W, C), C % 4 == 0
void vggish_bias_relu(const float* x, const float* b, float* y, int n, int H, int W, int C, int pool, hipStream_t s);
// out (n, 128) = clip(pca (emb - means), -2, 2), quantize: trunc((. + 2) * 63.75); pca_t = the matrix transposed
void vggish_postprocess(const float* emb, const float* pca_t, const float* means, float* out, int n, int quantize, hipStream_t s);

}  // namespace l3
