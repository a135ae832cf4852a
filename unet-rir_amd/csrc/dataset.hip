// dataset.hip - one launch assembles a training batch from the device-resident data set (gfx950): what
// DataGenerator.__getitem__ (datageneratorv2.py:64-102) builds on the host with two Python loops and three np.stack calls.
//
//   spec_in[b]  = bank[idx_in[b]]        spec_out[b] = bank[idx_out[b]]            feature rows [2][H][W], row_elems floats
//   emb[b][0]   = emb_bank[idx_in[b]]    emb[b][1]   = emb_bank[idx_out[b]]        (np.stack((emb_in, emb_out), axis=1), :91)
//   wav_true[b] = wav_bank[idx_out[b]]   room[b]     = room_bank[idx_out[b]]       (the target position: what the evaluation scores)
//
// A streaming copy.  A feature row is 184 KB contiguous at the reference geometry, so one workgroup per sample would leave most
// of the chip idle at B = 32: a row is cut into pieces of GATHER_PIECE floats (16 KB) and every (row, piece) pair is a workgroup -
// 2 * 32 * 12 = 768 workgroups at the reference batch, three per CU.  Lanes move 16 bytes each, consecutive lanes consecutive
// addresses; a thread issues its four loads before its four stores.  The 16-byte path needs row_elems % 4 == 0 and 16-byte
// aligned bases (then every row starts aligned); otherwise the same pieces are moved float by float, still coalesced.  The short
// rows (information vectors, room numbers) ride along in the first piece of their sample, the waveform rows of the target samples
// are workgroups of their own behind the feature pieces.
//
// Bank rows are read once per step and the outputs are read next by the stem convolution: non-temporal loads, ordinary stores
// (the line stays in L2 for the reader).  The ablation build can switch the loads to the default policy for the A/B of
// scripts/time_dataset.py.  Indices are trusted (include/unetrir.h): the generator range-checks its table on the host.
#include "kernels.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;
constexpr int GATHER_PIECE = GATHER_THREADS * GATHER_UNROLL * 4;      // floats per workgroup: 4096 = 16 KB

typedef float gather_f32x4 __attribute__((ext_vector_type(4)));

// piece `piece` of a row of n floats, src -> dst.  VEC: 16 bytes per lane (n % 4 == 0, both rows 16-byte aligned).
template <bool VEC, bool NT>
__device__ __forceinline__ void copy_piece(const float* __restrict__ src, float* __restrict__ dst, long long n, long long piece) {
    const long long base = piece * GATHER_PIECE;
    if constexpr (VEC) {
        const long long n4 = n >> 2, base4 = base >> 2;
        const gather_f32x4* s = reinterpret_cast<const gather_f32x4*>(src);
        gather_f32x4* d = reinterpret_cast<gather_f32x4*>(dst);
        gather_f32x4 v[GATHER_UNROLL];
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) {
            const long long i = base4 + k * GATHER_THREADS + threadIdx.x;
            if (i < n4) v[k] = NT ? __builtin_nontemporal_load(s + i) : s[i];
        }
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) {
            const long long i = base4 + k * GATHER_THREADS + threadIdx.x;
            if (i < n4) d[i] = v[k];
        }
    } else {
        float v[GATHER_UNROLL * 4];
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL * 4; ++k) {
            const long long i = base + k * GATHER_THREADS + threadIdx.x;
            if (i < n) v[k] = NT ? __builtin_nontemporal_load(src + i) : src[i];
        }
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL * 4; ++k) {
            const long long i = base + k * GATHER_THREADS + threadIdx.x;
            if (i < n) dst[i] = v[k];
        }
    }
}

struct GatherArgs {
    const float* bank; long long row_elems;
    const int32_t* emb_bank; int emb_len;
    const float* wav_bank; long long wav_len;
    const int32_t* room_bank;
    const int32_t* idx_in; const int32_t* idx_out; int B;
    float* spec_in; float* spec_out; int32_t* emb; float* wav_true; int32_t* room;
    int feat_pieces, wav_pieces;      // pieces of a feature row / of a waveform row (0 without a waveform bank)
    int vec_feat, vec_wav;
};

// 1-D grid: workgroups [0, 2 B feat_pieces) are the (row, piece) pairs of the feature rows - row j < B is input sample j, row
// j >= B is target sample j - B - and the wav_pieces * B workgroups behind them the pieces of the target waveforms.
template <bool NT>
__global__ __launch_bounds__(GATHER_THREADS) void gather_batch_kernel(const GatherArgs a) {
    const long long id = blockIdx.x, nfeat = 2LL * a.B * a.feat_pieces;
    if (id < nfeat) {
        const int j = (int)(id / a.feat_pieces), piece = (int)(id - (long long)j * a.feat_pieces);
        const bool target = j >= a.B;
        const int b = target ? j - a.B : j;
        const long long src = (target ? a.idx_out : a.idx_in)[b];          // wave-uniform: a scalar load
        const float* s = a.bank + src * a.row_elems;
        float* d = (target ? a.spec_out : a.spec_in) + (long long)b * a.row_elems;
        if (a.vec_feat) copy_piece<true, NT>(s, d, a.row_elems, piece);
        else copy_piece<false, NT>(s, d, a.row_elems, piece);
        if (piece == 0) {
            const int32_t* es = a.emb_bank + src * a.emb_len;
            int32_t* ed = a.emb + ((long long)b * 2 + (target ? 1 : 0)) * a.emb_len;
            for (int i = threadIdx.x; i < a.emb_len; i += GATHER_THREADS) ed[i] = es[i];
            if (target && a.room && threadIdx.x == 0) a.room[b] = a.room_bank[src];
        }
    } else {                                                                // only launched with a waveform bank
        const long long w = id - nfeat;
        const int b = (int)(w / a.wav_pieces), piece = (int)(w - (long long)b * a.wav_pieces);
        const long long src = a.idx_out[b];
        const float* s = a.wav_bank + src * a.wav_len;
        float* d = a.wav_true + (long long)b * a.wav_len;
        if (a.vec_wav) copy_piece<true, NT>(s, d, a.wav_len, piece);
        else copy_piece<false, NT>(s, d, a.wav_len, piece);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int unetrir_gather_batch_f32(const float* bank, long long N, long long row_elems, const int32_t* emb_bank, int emb_len,
                                        const float* wav_bank, long long wav_len, const int32_t* room_bank, const int32_t* idx_in,
                                        const int32_t* idx_out, int B, float* spec_in, float* spec_out, int32_t* emb, float* wav_true,
                                        int32_t* room, unetrir_stream_t stream) {
    if (!bank || !emb_bank || !idx_in || !idx_out || !spec_in || !spec_out || !emb) return UNETRIR_EINVAL;
    if (B <= 0 || N <= 0 || row_elems <= 0 || emb_len <= 0) return UNETRIR_EINVAL;
    if ((wav_bank == nullptr) != (wav_true == nullptr)) return UNETRIR_EINVAL;          // a waveform bank and its output come as a pair
    if (room && !room_bank) return UNETRIR_EINVAL;                                      // room numbers asked for without a bank
    if (wav_bank && wav_len <= 0) return UNETRIR_EINVAL;
    const long long feat_pieces = (row_elems + GATHER_PIECE - 1) / GATHER_PIECE;
    const long long wav_pieces = wav_bank ? (wav_len + GATHER_PIECE - 1) / GATHER_PIECE : 0;
    if (feat_pieces > 0x7fffffffLL || wav_pieces > 0x7fffffffLL) return UNETRIR_EINVAL;
    const long long blocks = (2 * feat_pieces + wav_pieces) * (long long)B;
    if (blocks > 0x7fffffffLL) return UNETRIR_EINVAL;                                   // grid limit
    GatherArgs a;
    a.bank = bank; a.row_elems = row_elems; a.emb_bank = emb_bank; a.emb_len = emb_len; a.wav_bank = wav_bank; a.wav_len = wav_len;
    a.room_bank = room_bank; a.idx_in = idx_in; a.idx_out = idx_out; a.B = B;
    a.spec_in = spec_in; a.spec_out = spec_out; a.emb = emb; a.wav_true = wav_true; a.room = room;
    a.feat_pieces = (int)feat_pieces; a.wav_pieces = (int)wav_pieces;
    a.vec_feat = (row_elems % 4 == 0) && aligned16(bank) && aligned16(spec_in) && aligned16(spec_out);
    a.vec_wav = wav_bank && (wav_len % 4 == 0) && aligned16(wav_bank) && aligned16(wav_true);
    const dim3 grid((unsigned)blocks);
    if (UNETRIR_ABL(UNETRIR_ABL_HOST(), 16384))          // ablation build only: default-policy loads
        hipLaunchKernelGGL(gather_batch_kernel<false>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(gather_batch_kernel<true>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
