// Exact signed Euclidean distance map of a batch of masks (mi_signed_distance): what the boundary loss of Kervadec et al. (MIDL 2019) weighs the
// probabilities with, computed where the mask lives.  The definition, restated from include/mi355seg.h:
//   G = (mask >= thresh); a NaN is background.  d2(q) = min over t in the OTHER set of |q - t|^2, an exact integer; pixels outside the image do not exist.
//   phi(q) = +sqrt(d2) outside G, -(sqrt(d2) - 1) inside G, formed in float64 and rounded to float32 once:
//   the float32 cast of edt(~G) * ~G - (edt(G) - 1) * G with scipy's distance_transform_edt.
//   G empty or the whole image: no contour, phi = 0 and d2 = 0 everywhere.
// Integers everywhere up to the final square root, no floating-point atomics: two calls give the same bits.  Nothing is read back.  Launches:
//   memset   the per-image foreground counters
//   columns  one lane per column, lanes along x, reading the mask itself: edt_sweep_column writes the vertical distance to the nearest foreground
//            pixel (low half) and to the nearest background pixel (high half) of the column as one 32-bit word; foreground pixels counted per image
//   rows     one workgroup per row, the row of g in LDS.  EVERY pixel queries the opposite set (edt_query).  The distance field is 1-Lipschitz, so
//            the scan lengths of neighbouring lanes differ by at most one step per pixel between them: a wave's lanes leave the loop within 63
//            steps of each other however far the contour is.  The per-image counts decide the phi = 0 case (uniform per workgroup).
#include <cmath>
#include "edt_common.h"

namespace {

constexpr long SD_MAX_GRID = 1l << 14;       // workgroups of a launch at most (64 per CU); beyond it a workgroup strides over the rows / columns
constexpr int SD_COL_THREADS = 64;           // the column sweep is a serial walk per lane: narrow workgroups spread the columns over more CUs

inline size_t sd_up(size_t n) { return (n + 255) & ~(size_t)255; }
inline bool sd_sizes_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && B <= 65535 && H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE; }
inline size_t sd_count_bytes(int B) { return sd_up((size_t)B * sizeof(unsigned)); }

__global__ __launch_bounds__(SD_COL_THREADS) void sdf_cols_kernel(const float* __restrict__ mask, float thresh, unsigned* __restrict__ g,
                                                                   unsigned* __restrict__ nfg, int B, int H, int W) {
    const long cols = (long)B * W;
    for (long c = (long)blockIdx.x * SD_COL_THREADS + threadIdx.x; c < cols; c += (long)gridDim.x * SD_COL_THREADS) {
        const int b = (int)(c / W), x = (int)(c % W);
        const float* m = mask + (long)b * H * W + x;
        unsigned n = 0u;
        edt_sweep_column(
            [&](int y) {
                const bool fg = m[(long)y * W] >= thresh;          // false for a NaN
                n += fg ? 1u : 0u;
                return fg ? 1u : 2u;
            },
            g + (long)b * H * W + x, H, W);
        if (n) atomicAdd(&nfg[b], n);
    }
}

__global__ __launch_bounds__(256) void sdf_rows_kernel(const unsigned* __restrict__ g, const unsigned* __restrict__ nfg, float* __restrict__ phi,
                                                       int* __restrict__ d2out, int* __restrict__ counts, int B, int H, int W) {
    __shared__ unsigned row[EDT_MAX_SIDE];
    const int tid = threadIdx.x;
    const long rows = (long)B * H;
    const unsigned npix = (unsigned)H * (unsigned)W;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {              // one row per workgroup unless the grid is capped
        const int b = (int)(r / H), y = (int)(r % H);
        const unsigned fg = nfg[b];
        if (counts && y == 0 && tid == 0) {
            counts[2 * b] = (int)fg;
            counts[2 * b + 1] = (int)(npix - fg);
        }
        const bool contour = fg != 0u && fg != npix;                   // uniform
        const long row0 = r * W;
        if (contour) {
            for (int x = tid; x < W; x += 256) row[x] = g[row0 + x];
            __syncthreads();
        }
        for (int x = tid; x < W; x += 256) {
            unsigned d = 0u;
            float v = 0.f;
            if (contour) {
                const bool inside = (row[x] & 0xffffu) == 0u;           // a foreground pixel is its own column's nearest foreground site
                d = edt_query(row, x, W, inside ? 16 : 0);
                const double s = __dsqrt_rn((double)d);
                v = (float)(inside ? 1.0 - s : s);          // 1 - s: -(s - 1) with the +0 the published line gives at s = 1
            }
            phi[row0 + x] = v;
            if (d2out) d2out[row0 + x] = (int)d;
        }
        __syncthreads();                                               // the next row overwrites `row`
    }
}

}  // namespace

extern "C" size_t mi_signed_distance_workspace(int B, int H, int W) {
    if (!sd_sizes_ok(B, H, W)) return 0;
    return sd_count_bytes(B) + sd_up((size_t)B * H * W * sizeof(unsigned));
}

extern "C" int mi_signed_distance(const float* mask, float thresh, float* phi, int32_t* d2, int32_t* counts, int B, int H, int W, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    MI_REQUIRE(mask && phi && workspace, "mi_signed_distance: null operand");
    MI_REQUIRE(B > 0 && H > 0 && W > 0, "mi_signed_distance: bad dimension (B %d, masks %d x %d)", B, H, W);
    MI_REQUIRE(sd_sizes_ok(B, H, W), "mi_signed_distance: B %d, masks %d x %d beyond the limits (B <= 65535, sides <= %d)", B, H, W, EDT_MAX_SIDE);
    MI_REQUIRE(std::isfinite(thresh), "mi_signed_distance: thresh is not finite");
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "mi_signed_distance: workspace must be 4-byte aligned");
    const size_t need = mi_signed_distance_workspace(B, H, W);
    if (workspace_bytes < need) return mi_set_error(MI_ENOMEM, "mi_signed_distance: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    unsigned* nfg = reinterpret_cast<unsigned*>(workspace);
    unsigned* g = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(workspace) + sd_count_bytes(B));
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)B * H, col_wgs = ((long)B * W + SD_COL_THREADS - 1) / SD_COL_THREADS;
    if (hipMemsetAsync(nfg, 0, (size_t)B * sizeof(unsigned), s) != hipSuccess) return mi_set_error(MI_EHIP, "mi_signed_distance: memset failed");
    hipLaunchKernelGGL(sdf_cols_kernel, dim3((unsigned)(col_wgs < SD_MAX_GRID ? col_wgs : SD_MAX_GRID)), dim3(SD_COL_THREADS), 0, s, mask, thresh, g, nfg, B,
                       H, W);
    MI_CHECK_LAUNCH("mi_signed_distance columns");
    hipLaunchKernelGGL(sdf_rows_kernel, dim3((unsigned)(rows < SD_MAX_GRID ? rows : SD_MAX_GRID)), dim3(256), 0, s, (const unsigned*)g, (const unsigned*)nfg,
                       phi, reinterpret_cast<int*>(d2), reinterpret_cast<int*>(counts), B, H, W);
    MI_CHECK_LAUNCH("mi_signed_distance rows");
    return MI_OK;
}
