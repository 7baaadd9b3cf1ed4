// The GroupNorm apply arithmetic shared by norm_apply_rows_kernel (norm_kernels.hip) and gn_shortcut_kernel (gn_shortcut.hip):
// both compile these expressions, so the two routes of ResBlockUp's bn1 give the same bits.
#pragma once
#include "common.h"

namespace cslgan {

// Partials left by a conv epilogue (cslgan_conv_t.gn_part): per slot the sum of its cnt / n_part values and their sum of squares
// about the slot's own mean — combined exactly (Chan et al.): M2 = sum_b M2_b + n_b (mean_b - mean)^2.  Threads i < n_groups of
// a 256-thread workgroup leave (mean, centred sum of squares) of row group sr in s_st[2 * i + {0, 1}]; with `publish` they also
// write the final (sum x, centred sum of squares) pairs to stats_out (nullable).  The caller synchronises before reading s_st.
__device__ __forceinline__ void gn_combine_chan(const float* __restrict__ part, long long sr, int n_part, int n_groups, float cnt,
                                                float* s_st, float* __restrict__ stats_out, bool publish) {
    for (int i = threadIdx.x; i < n_groups; i += 256) {
        float sum = 0.f;
        for (int b = 0; b < n_part; ++b) sum += part[((sr * n_part + b) * n_groups + i) * 2];
        const float nb = cnt / (float)n_part, mean_all = sum / cnt;
        float css = 0.f;
        for (int b = 0; b < n_part; ++b) {
            const float* q = part + ((sr * n_part + b) * n_groups + i) * 2;
            const float dm = q[0] / nb - mean_all;
            css += q[1] + nb * dm * dm;
        }
        s_st[2 * i] = mean_all;
        s_st[2 * i + 1] = css;
        if (stats_out && publish) {
            stats_out[2 * (sr * n_groups + i)] = sum;
            stats_out[2 * (sr * n_groups + i) + 1] = css;
        }
    }
}

// (mean, rstd) of group g from the pairs gn_combine_chan left
__device__ __forceinline__ void gn_group_stat(const float* s_st, int g, float inv_cnt, float eps, float& mean, float& rstd) {
    mean = s_st[2 * g];
    rstd = rsqrtf(s_st[2 * g + 1] * inv_cnt + eps);
}

__device__ __forceinline__ float gn_apply(float x, float mean, float rstd, float ga, float be, int relu) {
    const float t = (x - mean) * rstd * ga + be;
    return (relu && t < 0.f) ? 0.f : t;
}

}  // namespace cslgan
