// k_resample_bank.hip -- the device side of the resampler bank (api_resampler_bank.cpp): the streaming form of the
// rational-position converter (audiofile.hpp, rational_file in k_resample.hip) for N live channels whose filter history stays in
// HBM between pushes.
//
// Output n of a channel sits at ip = (n p) div q with phase r = (n p) mod q and sums the phase's ready-made weights against the
// inputs x[ip + m], first[r] <= m < first[r] + count[r], in ascending m, in double precision; it is final as soon as its last
// possible tap ip + m_hi has arrived.  The host knows every count, so it plans a push alone and uploads one ResamplerRow per channel
// that received samples (or is being finished); nothing here is read back.  For a channel, cat = carried ++ fresh holds the signal
// from index c0 on: carried = x[c0, L) with c0 = max(0, ip(next output) + m_lo), fresh = x[L, L + n).
//
//   convert   one workgroup per channel, run of at most `run` (<= 256) consecutive outputs inside the period of q outputs, and group
//             of kResamplerBankPeriods consecutive periods, found by the uniform binary search of bank_stage.  Outputs n and n + q
//             have the SAME phase, hence the same weights, and their inputs lie exactly p samples apart (rational_file's lever): a
//             lane loads each of its weights once and uses it for its output in every period of the group -- one second of
//             44.1 kHz is four periods of 1 378 outputs.  (First version: one output per lane, every weight loaded once per
//             output, 17 GB a push of 1 024 channels: 1.13 ms against 0.64 ms for this one)  Each
//             period's input range goes from cat into its own LDS block -- indices outside [0, end) as +0.0f, int16 converted
//             at the load -- in rational_file's padded layout (a pad word per eight samples: lanes eight samples apart on
//             distinct banks); a lane's taps sit at the same offset in every block.  A product with a staged +0.0f leaves the sum
//             as it is (it is never -0.0), so the result has the bits of the host loop, which skips such taps.  Consecutive
//             outputs have phases p mod q apart: contiguous weights across the lanes for 44.1 kHz -> 5512 Hz, a gather for
//             48 kHz -> 5512 Hz.  A row that emits less than a period has one period per unit and takes the one-period loop.
//             Where q is small (below two runs: integer ratios have q = 1) positions inside a period would leave lanes idle, so
//             there the bank's `period` is longer than any call's outputs: a unit is a run of CONSECUTIVE outputs, one per lane,
//             in the one-period loop -- the first version's form; lanes of one phase then share their weight loads.
//   commit    behind it, one workgroup per row: what the channel carries on.  A channel that emitted nothing appends its fresh
//             samples behind the ones it has (c0 stays).  Otherwise cat[c1 - c0, ...) moves to the front, and since that would move
//             the carried samples left over themselves the channel has TWO carried buffers, as in k_stream_bank.hip: the launch
//             reads side s and writes side s ^ 1, and the host flips its record of the side.  No launch reads what another
//             workgroup of it may write.  A finished channel carries nothing and has no commit.
#include "internal.hpp"

namespace lbad {
namespace {

constexpr uint32_t kRsThreads = 256;
constexpr uint32_t kRsMaxGrid = 1u << 16;        // most workgroups of a launch (its workgroups stride over the rest)
constexpr uint32_t kRsStride = kResamplerBankStageMax + kResamplerBankStageMax / 8 + 1;   // words of the padded staged range
static_assert(kResamplerBankMaxRun == kRsThreads, "one lane per output of a run");

// the row whose units hold unit u of the push: the last r with rows[r].first_unit <= u.  A row that emits nothing shares its
// `first_unit` with the row behind it, and the last row's is the push's total when it has none, so the answer always has the unit.
__device__ __forceinline__ uint32_t rs_row_of(const ResamplerRow* __restrict__ rows, uint32_t n_rows, uint32_t u) {
    uint32_t lo = 0, hi = n_rows;                // rows[lo].first_unit <= u < rows[hi].first_unit (hi == n_rows: none)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rows[mid].first_unit <= u) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float* rs_carry(const ResamplerBankDev& b, uint32_t side, uint32_t channel) {
    return b.carry + ((uint64_t)side * b.n_channels + channel) * b.carry_stride;
}

// sample i of the push's block: float32, or int16 read as the batch kernels read it
template <bool Int16>
__device__ __forceinline__ float rs_fresh(const void* __restrict__ fresh, uint64_t i) {
    if (Int16) return (float)static_cast<const int16_t*>(fresh)[i] * (1.0f / 32768.0f);
    return static_cast<const float*>(fresh)[i];
}

// sample k (0 <= k < row.end) of the row's channel: carried below L, fresh from L on
template <bool Int16>
__device__ __forceinline__ float rs_sample(const ResamplerRow& row, const float* __restrict__ carried, const void* __restrict__ fresh,
                                           uint64_t k) {
    return k < row.L ? carried[k - row.c0] : rs_fresh<Int16>(fresh, row.fresh_at + (k - row.L));
}

// (a global-memory pointer, said so: a generic one makes every weight a flat load that also counts as an LDS access)
typedef const __attribute__((address_space(1))) double* rs_weight_p;

// the taps of one lane's outputs in KK periods: weight j (rows q apart) against staged sample s + j of every period's block, in
// ascending j; eight taps' weights and samples are requested together
template <int KK>
__device__ __forceinline__ void rs_taps(const float (*__restrict__ s_in)[kRsStride], uint32_t s, rs_weight_p w, uint64_t q, uint32_t cnt,
                                        double (&acc)[kResamplerBankPeriods]) {
    uint32_t j = 0;
    for (; j + 8 <= cnt; j += 8, s += 8, w += 8 * q) {
        double wv[8];
        float x[KK][8];
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) wv[t] = w[(size_t)t * q];
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) {
            const uint32_t at = (s + t) + ((s + t) >> 3);
#pragma unroll
            for (int k = 0; k < KK; ++k) x[k][t] = s_in[k][at];
        }
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t)
#pragma unroll
            for (int k = 0; k < KK; ++k) acc[k] += wv[t] * (double)x[k][t];
    }
    for (; j < cnt; ++j, ++s, w += q) {
        const double wv = *w;
#pragma unroll
        for (int k = 0; k < KK; ++k) acc[k] += wv * (double)s_in[k][s + (s >> 3)];
    }
}

template <bool Int16>
__global__ __launch_bounds__(kRsThreads) void resampler_bank_convert_kernel(ResamplerBankDev b, const ResamplerRow* __restrict__ rows,
                                                                            uint32_t n_rows, const void* __restrict__ fresh,
                                                                            uint32_t n_units, float* __restrict__ out) {
    constexpr uint32_t K = kResamplerBankPeriods;
    __shared__ float s_in[K][kRsStride];
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const ResamplerRow row = rows[rs_row_of(rows, n_rows, u)];
        // the row's units: runs inside the period (the period itself where the row emits less), then groups of K periods
        const uint32_t in_period = row.emit < b.period ? row.emit : (uint32_t)b.period;
        const uint32_t runs = (in_period + b.run - 1) / b.run, lu = u - row.first_unit;
        const uint32_t t0 = (lu % runs) * b.run, k0 = (lu / runs) * K;       // first position of the run, first period of the group
        const uint32_t lanes = in_period - t0 < b.run ? in_period - t0 : b.run;
        // output out_first + j sits at ip0 + (r0 + j p) div q, phase (r0 + j p) mod q (j p < 2^55); j + q: p further, same phase
        const uint64_t a_first = (uint64_t)row.r0 + (uint64_t)t0 * b.p, a_last = a_first + (uint64_t)(lanes - 1) * b.p;
        const uint64_t ip_first = row.ip0 + a_first / b.q;                  // of position t0 in the row's first period
        const uint32_t len = (uint32_t)(a_last / b.q - a_first / b.q) + b.m_span;    // a period's staged range
        __syncthreads();                                                    // s_in is reused by consecutive units
        if (len > kResamplerBankStageMax) continue;                         // (uniform; never: the host sizes `run` for the range)
        const float* __restrict__ carried = rs_carry(b, row.side, row.channel);
        uint32_t n_k[K];                                                    // this run's outputs in period k0 + k
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) {
            const uint64_t j0 = (uint64_t)(k0 + k) * b.period + t0;         // (period != q: k0 + k = 0 is the one period there is)
            n_k[k] = j0 < row.emit ? (uint32_t)(row.emit - j0 < lanes ? row.emit - j0 : lanes) : 0u;
            if (n_k[k] == 0) continue;                                      // (uniform)
            const long kbase = (long)(ip_first + (uint64_t)(k0 + k) * b.p) + (long)b.m_min;
            for (uint32_t i = threadIdx.x; i < len; i += kRsThreads) {
                const long x = kbase + (long)i;
                s_in[k][i + (i >> 3)] = x >= 0 && (uint64_t)x < row.end ? rs_sample<Int16>(row, carried, fresh, (uint64_t)x) : 0.0f;
            }
        }
        __syncthreads();
        if (threadIdx.x >= lanes) continue;
        const uint64_t a = a_first + (uint64_t)threadIdx.x * b.p, r = a % b.q;
        const long ip = (long)(row.ip0 + a / b.q), m0 = (long)b.first[r];
        const uint32_t cnt = b.count[r];
        rs_weight_p w = (rs_weight_p)(b.w + (size_t)(m0 - (long)b.m_min) * b.q + r);
        const uint32_t s = (uint32_t)(ip + m0 - ((long)ip_first + (long)b.m_min));    // the first tap's staged sample, in every block
        double acc[K];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) acc[k] = 0.0;
        // (an output behind the row's last walks its block all the same: read -- stale words at worst --, never stored)
        if (n_k[1] == 0) rs_taps<1>(s_in, s, w, b.q, cnt, acc);             // (uniform)
        else rs_taps<(int)K>(s_in, s, w, b.q, cnt, acc);
        const double wsum = b.wsum[r];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k)
            if (threadIdx.x < n_k[k])
                out[row.out_at + (uint64_t)(k0 + k) * b.period + t0 + threadIdx.x] = (float)(wsum != 0.0 ? acc[k] / wsum : 0.0);
    }
}

// what every row's channel carries on: x[c1, end)
template <bool Int16>
__global__ __launch_bounds__(kRsThreads) void resampler_bank_commit_kernel(ResamplerBankDev b, const ResamplerRow* __restrict__ rows,
                                                                           uint32_t n_rows, const void* __restrict__ fresh) {
    for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const ResamplerRow row = rows[r];
        float* cur = rs_carry(b, row.side, row.channel);
        if (row.emit == 0) {                     // c1 == c0: the fresh samples go behind the L - c0 carried ones
            float* dst = cur + (row.L - row.c0);
            for (uint32_t i = threadIdx.x; i < row.n; i += kRsThreads) dst[i] = rs_fresh<Int16>(fresh, row.fresh_at + i);
        } else {
            float* dst = rs_carry(b, row.side ^ 1u, row.channel);
            const uint32_t len = (uint32_t)(row.end - row.c1);
            for (uint32_t i = threadIdx.x; i < len; i += kRsThreads) dst[i] = rs_sample<Int16>(row, cur, fresh, row.c1 + i);
        }
    }
}

}  // namespace

hipError_t launch_resampler_bank_convert(const ResamplerBankDev& b, const ResamplerRow* d_rows, uint32_t n_rows, const void* d_fresh,
                                         uint32_t format, uint32_t n_units, float* d_out, hipStream_t stream) {
    if (n_rows == 0 || n_units == 0) return hipSuccess;
    const dim3 grid(strided_grid(n_units, kRsMaxGrid)), block(kRsThreads);
    if (format)
        hipLaunchKernelGGL(resampler_bank_convert_kernel<true>, grid, block, 0, stream, b, d_rows, n_rows, d_fresh, n_units, d_out);
    else
        hipLaunchKernelGGL(resampler_bank_convert_kernel<false>, grid, block, 0, stream, b, d_rows, n_rows, d_fresh, n_units, d_out);
    return hipGetLastError();
}

hipError_t launch_resampler_bank_commit(const ResamplerBankDev& b, const ResamplerRow* d_rows, uint32_t n_rows, const void* d_fresh,
                                        uint32_t format, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    const dim3 grid(strided_grid(n_rows, kRsMaxGrid)), block(kRsThreads);
    if (format)
        hipLaunchKernelGGL(resampler_bank_commit_kernel<true>, grid, block, 0, stream, b, d_rows, n_rows, d_fresh);
    else
        hipLaunchKernelGGL(resampler_bank_commit_kernel<false>, grid, block, 0, stream, b, d_rows, n_rows, d_fresh);
    return hipGetLastError();
}

}  // namespace lbad
