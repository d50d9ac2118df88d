// Connected components of a batch of binary masks (mi_label_components) and the lesion-wise detection counts built on them (mi_lesion_score,
// TEST.LESION_METRICS / TEST.MASK_MIN_AREA / TEST.MASK_KEEP_LARGEST).  The definitions are in include/mi355seg.h.  Label-equivalence
// union-find on row runs, in global memory:
//   rows      one workgroup per row: the 64-bit ballots of the row (one bit per pixel) go to the workspace; every foreground pixel's parent is
//             the linear index of the first pixel of its run, background is -1.  A run may cross any number of ballot words.
//   merge     every run start looks at the row above over [x0 - d, x1 + d] (d = 0 for connectivity 4, 1 for 8) and unites its root with the
//             root of each run it touches there: one union per touching pair of runs
//   flatten   every run start finds its root, the run copies it; one integer atomic per run adds the run length to area[root]
// mi_label_components then numbers the roots in raster order (a row's root count, a scan over the rows of an image, the rank within the row)
// and writes labels / roots; mi_lesion_score runs P = (pred == cls) and G = (label == cls) through the same three launches as 2 B planes, then
//   select    component counts, largest areas and, per image, atomicMax of (area << 32) | ~root over the components of P of at least min_area
//   hits      P' per pixel (`filtered`), and one integer atomic per run: the popcount of the other mask's ballot under the run
//   count     the components of P', the true positives, the detected lesions
//   finish    the row of 12 integers
// Invariant behind every loop over parents: parent[i] <= i at all times - a run start is at or before its pixels, and the only later writes are
// atomicMin with a smaller index and the flatten store of a root.  So a walk along parents strictly decreases and ends after fewer steps than the
// image has pixels, whatever other workgroups do meanwhile.  No workgroup waits on another: no flags, no spinning on a value somebody else will
// write.  The root of a component is its smallest linear index, its first pixel in raster order, whatever the order of the unions: every output
// bit is equal run to run.  Integers only.
#include "mi_common.h"

namespace {

typedef unsigned long long u64;

constexpr int CC_MAX_SIDE = 4096;
constexpr int CC_MAX_WORDS = CC_MAX_SIDE / 64;
constexpr long CC_MAX_GRID = 1l << 14;       // workgroups of a launch at most (64 per CU); beyond it a workgroup strides over the rows
constexpr int CC_ACC = 16;                   // per image: the 12 output integers in their order, then 12 = the packed selection maximum
constexpr int CC_ACC_BEST = 12;
static_assert(MI_LESION_INTS == 12 && CC_ACC > CC_ACC_BEST, "ints row: 12 fields");

inline size_t cc_up(size_t n) { return (n + 255) & ~(size_t)255; }
inline int cc_words(int W) { return (W + 63) / 64; }

struct CcWs {
    u64* acc;            // [B][CC_ACC]                        (lesion score only)
    u64* bits;           // [planes][H][words]                 the row ballots
    int* rowcnt;         // [planes][H]                        roots of a row, then (scan) roots of the rows before it
    int* parent;         // [planes][H][W]
    int* area;           // [planes][H][W]                     read at roots only; the component's number in mi_label_components
    int* hit;            // [planes][H][W]                     (lesion score only)
    size_t bytes;
};
inline CcWs cc_layout(void* base, long planes, int H, int W, bool lesion) {
    CcWs w;
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);      // integer arithmetic: the size query lays out from a null base
    size_t o = 0;
    const size_t px = (size_t)planes * H * W;
    w.acc = reinterpret_cast<u64*>(p + o);
    o += lesion ? cc_up((size_t)(planes / 2) * CC_ACC * sizeof(u64)) : 0;
    w.bits = reinterpret_cast<u64*>(p + o);
    o += cc_up((size_t)planes * H * cc_words(W) * sizeof(u64));
    w.rowcnt = reinterpret_cast<int*>(p + o);
    o += cc_up((size_t)planes * H * sizeof(int));
    w.parent = reinterpret_cast<int*>(p + o);
    o += cc_up(px * sizeof(int));
    w.area = reinterpret_cast<int*>(p + o);
    o += cc_up(px * sizeof(int));
    w.hit = reinterpret_cast<int*>(p + o);
    o += lesion ? cc_up(px * sizeof(int)) : 0;
    w.bytes = o;
    return w;
}

inline bool cc_sizes_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && B <= 65535 && H <= CC_MAX_SIDE && W <= CC_MAX_SIDE; }

// The two masks of a launch: planes below `n8` are uint8 planes of `m8`, the others int64 planes of `m64`.
struct CcSrc {
    const uint8_t* m8;
    const long long* m64;
    int n8, cls;
};
__device__ __forceinline__ bool cc_fg(const CcSrc& s, long plane, long hw, long i) {
    return plane < s.n8 ? s.m8[plane * hw + i] == s.cls : s.m64[(plane - s.n8) * hw + i] == s.cls;
}

__device__ __forceinline__ unsigned cc_wave_sum(unsigned v) {
    for (int m = 32; m > 0; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
    return v;
}
__device__ __forceinline__ u64 cc_wave_max64(u64 v) {
    for (int m = 32; m > 0; m >>= 1) {
        const u64 o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}
// The sum of `v` over the wave, added to *cell by one lane.  Every lane of the wave calls.
__device__ __forceinline__ void cc_wave_add(u64* cell, unsigned v, int lane) {
    v = cc_wave_sum(v);
    if (lane == 0 && v) atomicAdd(cell, (u64)v);
}

// Bit scans over the ballot words `w` of a row (`nw` words; bits at and beyond W are 0).
// First pixel of the run that holds foreground pixel x: at most nw steps.
__device__ __forceinline__ int cc_run_start(const u64* w, int x) {
    int wi = x >> 6;
    u64 inv = ~w[wi] & ((1ull << (x & 63)) - 1ull);
    while (inv == 0ull) {
        if (wi == 0) return 0;
        inv = ~w[--wi];
    }
    return wi * 64 + 64 - __clzll((long long)inv);
}
// Last pixel of the run that holds foreground pixel x: at most nw steps.
__device__ __forceinline__ int cc_run_end(const u64* w, int x, int nw) {
    int wi = x >> 6;
    u64 inv = ~w[wi] & (~0ull << (x & 63));
    while (inv == 0ull) {
        if (++wi == nw) return nw * 64 - 1;
        inv = ~w[wi];
    }
    return wi * 64 + __ffsll((long long)inv) - 2;
}
// First foreground pixel at or after p, or INT_MAX: at most nw steps.
__device__ __forceinline__ int cc_next_set(const u64* w, int p, int nw) {
    int wi = p >> 6;
    if (wi >= nw) return 0x7fffffff;
    u64 m = w[wi] & (~0ull << (p & 63));
    while (m == 0ull) {
        if (++wi == nw) return 0x7fffffff;
        m = w[wi];
    }
    return wi * 64 + __ffsll((long long)m) - 1;
}
// Foreground pixels in [x0, x1]: at most nw steps.
__device__ __forceinline__ int cc_popcount(const u64* w, int x0, int x1) {
    const int w0 = x0 >> 6, w1 = x1 >> 6;
    int n = 0;
    for (int wi = w0; wi <= w1; ++wi) {
        u64 m = w[wi];
        if (wi == w0) m &= ~0ull << (x0 & 63);
        if (wi == w1) m &= ~0ull >> (63 - (x1 & 63));
        n += __popcll(m);
    }
    return n;
}
__device__ __forceinline__ bool cc_bit(const u64* w, int x) { return (w[x >> 6] >> (x & 63)) & 1ull; }
__device__ __forceinline__ bool cc_is_start(const u64* w, int x) { return cc_bit(w, x) && (x == 0 || !cc_bit(w, x - 1)); }

// A parent cell as another workgroup's atomicMin left it: a device-scope load, never a line this CU cached earlier.
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of i.  Terminates: parent[i] <= i always, so i strictly decreases until parent[i] == i - fewer steps than the image has pixels.
__device__ __forceinline__ int cc_find(const int* parent, int i) {
    for (int p = cc_load(parent + i); p != i; p = cc_load(parent + i)) i = p;
    return i;
}

// Unites the components of a and b, lock-free.  Terminates: each round either ends, or replaces max(a, b) by a strictly smaller index (the value
// atomicMin returned is below the cell's own index whenever it is not that index), so there are fewer rounds than the image has pixels.  Nothing
// here waits for another lane: a lost race only hands this lane a smaller index to go on from.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);          // device scope: the cell may belong to a row of another workgroup, on another XCD
        if (old == a) return;                              // a was a root and now hangs under b
        a = old;                                           // somebody moved the cell first: a's tree hangs under min(old, b); unite those two
    }
}

// The ballot words of one row from the workspace into LDS.  Every thread calls; ends with a barrier.
__device__ __forceinline__ void cc_load_words(u64* dst, const u64* src, int nw) {
    if ((int)threadIdx.x < nw) dst[threadIdx.x] = src[threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(256) void cc_rows_kernel(CcSrc src, long planes, int H, int W, u64* __restrict__ bits, int* __restrict__ parent,
                                                      int* __restrict__ area, int* __restrict__ hit) {
    __shared__ u64 words[CC_MAX_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (W + 63) >> 6;
    const long rows = planes * H, hw = (long)H * W;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {              // one row per workgroup unless the grid is capped
        const long plane = r / H;
        const int y = (int)(r % H);
        for (int x0 = 0; x0 < W; x0 += 256) {                          // uniform trip count: the ballots need every lane
            const int x = x0 + tid;
            const u64 m = __ballot(x < W && cc_fg(src, plane, hw, (long)y * W + x));
            const int wi = (x0 >> 6) + wave;
            if (lane == 0 && wi < nw) {
                words[wi] = m;
                bits[r * nw + wi] = m;
            }
        }
        __syncthreads();
        for (int x = tid; x < W; x += 256) {
            const long i = r * W + x;
            int p = -1;
            if (cc_bit(words, x)) {
                const int s = cc_run_start(words, x);
                p = y * W + s;
                if (s == x) {                                          // only a run start can become a root: the cells the atomics add to
                    area[i] = 0;
                    if (hit) hit[i] = 0;
                }
            }
            parent[i] = p;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(long planes, int H, int W, int d, const u64* __restrict__ bits, int* __restrict__ parent) {
    __shared__ u64 cur[CC_MAX_WORDS], up[CC_MAX_WORDS];
    const int tid = threadIdx.x, nw = (W + 63) >> 6;
    const long rows = planes * H, hw = (long)H * W;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long plane = r / H;
        const int y = (int)(r % H);
        if (y == 0) continue;                                          // uniform
        if (tid < nw) {
            cur[tid] = bits[r * nw + tid];
            up[tid] = bits[(r - 1) * nw + tid];
        }
        __syncthreads();
        int* par = parent + plane * hw;
        for (int x = tid; x < W; x += 256) {
            if (!cc_is_start(cur, x)) continue;
            const int x1 = cc_run_end(cur, x, nw);
            const int hi = min(x1 + d, W - 1);
            // the runs of the row above that touch [x - d, x1 + d]: p moves past one whole run per round, at most W / 2 + 1 rounds
            for (int p = max(x - d, 0);;) {
                const int q = cc_next_set(up, p, nw);
                if (q > hi) break;
                cc_union(par, y * W + x, (y - 1) * W + q);
                p = cc_run_end(up, q, nw) + 2;                         // the pixel after a run is background
            }
        }
        __syncthreads();
    }
}

// Every pixel gets its root.  Parents of other rows may be read while their workgroup overwrites them with their root: either value is an ancestor
// of the cell and below its index, so cc_find still ends at the root.  rowcnt (may be NULL): the roots of each row.
__global__ __launch_bounds__(256) void cc_flatten_kernel(long planes, int H, int W, const u64* __restrict__ bits, int* __restrict__ parent,
                                                         int* __restrict__ area, int* __restrict__ rowcnt) {
    __shared__ u64 words[CC_MAX_WORDS];
    __shared__ int root[CC_MAX_SIDE];
    __shared__ unsigned nroot;
    const int tid = threadIdx.x, lane = tid & 63, nw = (W + 63) >> 6;
    const long rows = planes * H, hw = (long)H * W;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long plane = r / H;
        const int y = (int)(r % H);
        if (tid == 0) nroot = 0u;
        cc_load_words(words, bits + r * nw, nw);
        int* par = parent + plane * hw;
        for (int x0 = 0; x0 < W; x0 += 256) {                          // uniform trip count: the wave sum needs every lane
            const int x = x0 + tid;
            unsigned is_root = 0u;
            if (x < W && cc_is_start(words, x)) {
                const int rt = cc_find(par, y * W + x);
                root[x] = rt;
                is_root = rt == y * W + x ? 1u : 0u;
                atomicAdd(area + plane * hw + rt, cc_run_end(words, x, nw) - x + 1);      // one atomic per run, not per pixel
            }
            is_root = cc_wave_sum(is_root);
            if (lane == 0 && is_root) atomicAdd(&nroot, is_root);
        }
        __syncthreads();
        for (int x = tid; x < W; x += 256)
            if (cc_bit(words, x)) par[(long)y * W + x] = root[cc_run_start(words, x)];
        if (tid == 0 && rowcnt) rowcnt[r] = (int)nroot;
        __syncthreads();
    }
}

// One workgroup per image: rowcnt becomes the number of roots in the rows before each row, counts[b] the number of components.
__global__ __launch_bounds__(256) void cc_scan_kernel(int H, int* __restrict__ rowcnt, int* __restrict__ counts) {
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (H + 255) / 256;
    int* rc = rowcnt + (long)blockIdx.x * H;
    const int y0 = tid * per, y1 = min(y0 + per, H);
    int s = 0;
    for (int y = y0; y < y1; ++y) s += rc[y];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        counts[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int y = y0; y < y1; ++y) {
        const int v = rc[y];
        rc[y] = run;
        run += v;
    }
}

// The number of every root: 1 + the roots before it in raster order, into num[root].
__global__ __launch_bounds__(256) void cc_number_kernel(long planes, int H, int W, const int* __restrict__ parent, const int* __restrict__ rowoff,
                                                        int* __restrict__ num) {
    __shared__ u64 words[CC_MAX_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long rows = planes * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int y = (int)(r % H);
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            const u64 m = __ballot(x < W && parent[r * W + x] == y * W + x);
            if (lane == 0) words[(x0 >> 6) + wave] = m;                // the last round may write words past W: they are 0 and in bounds
        }
        __syncthreads();
        for (int x = tid; x < W; x += 256)
            if (cc_bit(words, x)) num[r * W + x] = rowoff[r] + 1 + (x ? cc_popcount(words, 0, x - 1) : 0);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cc_write_kernel(long planes, long hw, const int* __restrict__ parent, const int* __restrict__ num,
                                                       int* __restrict__ labels, int* __restrict__ roots) {
    const long n = planes * hw;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int rt = parent[i];
        if (roots) roots[i] = rt;
        if (labels) labels[i] = rt < 0 ? 0 : num[i / hw * hw + rt];
    }
}

struct CcFilter {
    int min_area, keep_largest, permille;
};
__device__ __forceinline__ u64 cc_pack(int area, int root) { return ((u64)(unsigned)area << 32) | (u64)(~(unsigned)root); }
__device__ __forceinline__ bool cc_kept(const CcFilter& f, int area, int root, u64 best) {
    return area >= f.min_area && (!f.keep_largest || cc_pack(area, root) == best);
}
__device__ __forceinline__ bool cc_overlaps(const CcFilter& f, int hit, int area) {
    return hit >= 1 && 1000ll * (long long)hit >= (long long)f.permille * (long long)area;
}

// Planes [0, B) are P, [B, 2 B) are G.  Component counts, largest areas, and the largest component of P of at least min_area; a tie goes to the
// smaller root (the larger ~root), the component whose first pixel comes first.
__global__ __launch_bounds__(256) void cc_select_kernel(int B, int H, int W, CcFilter f, const int* __restrict__ parent, const int* __restrict__ area,
                                                        u64* __restrict__ acc) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long rows = 2l * B * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long plane = r / H;
        const int y = (int)(r % H), is_g = plane >= B ? 1 : 0;
        u64* a = acc + (plane - (is_g ? B : 0)) * CC_ACC;
        unsigned n = 0u;
        u64 big = 0ull, best = 0ull;
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            if (x < W && parent[r * W + x] == y * W + x) {
                const int ar = area[r * W + x];
                ++n;
                big = max(big, (u64)ar);
                if (!is_g && ar >= f.min_area) best = max(best, cc_pack(ar, y * W + x));
            }
        }
        cc_wave_add(a + 3 + 2 * is_g, n, lane);
        big = cc_wave_max64(big);
        best = cc_wave_max64(best);
        if (lane == 0 && big) atomicMax(a + 8 + is_g, big);
        if (lane == 0 && best) atomicMax(a + CC_ACC_BEST, best);
    }
}

// One workgroup per image row: P' (and `filtered`), the pixel counts, and per run the pixels of the other mask under it.
__global__ __launch_bounds__(256) void cc_hits_kernel(int B, int H, int W, int cls, CcFilter f, const u64* __restrict__ bits,
                                                      const int* __restrict__ parent, const int* __restrict__ area, int* __restrict__ hit,
                                                      u64* __restrict__ acc, uint8_t* __restrict__ filtered) {
    __shared__ u64 wp[CC_MAX_WORDS], wg[CC_MAX_WORDS], wf[CC_MAX_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (W + 63) >> 6;
    const long rows = (long)B * H, hw = (long)H * W;
    const uint8_t off = cls == 0 ? 1 : 0;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long b = r / H, rg = r + rows;                           // the same row of the G plane
        const int y = (int)(r % H);
        u64* a = acc + b * CC_ACC;
        const u64 best = a[CC_ACC_BEST];
        const int* area_p = area + b * hw;
        if (tid < nw) {
            wp[tid] = bits[r * nw + tid];
            wg[tid] = bits[rg * nw + tid];
        }
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            bool keep = false;
            if (x < W) {
                const int rt = parent[r * W + x];
                keep = rt >= 0 && cc_kept(f, area_p[rt], rt, best);
                if (filtered) filtered[r * W + x] = keep ? (uint8_t)cls : off;
            }
            const u64 m = __ballot(keep);
            if (lane == 0) wf[(x0 >> 6) + wave] = m;
        }
        __syncthreads();
        unsigned n_p = 0u, n_f = 0u, n_g = 0u, n_fg = 0u;
        if (tid < nw) {
            n_p = __popcll(wp[tid]);
            n_f = __popcll(wf[tid]);
            n_g = __popcll(wg[tid]);
            n_fg = __popcll(wf[tid] & wg[tid]);
        }
        if (wave == 0) {                                               // nw <= 64: the words sit in the first wave
            cc_wave_add(a + 0, n_p, lane);
            cc_wave_add(a + 1, n_f, lane);
            cc_wave_add(a + 2, n_g, lane);
            cc_wave_add(a + 10, n_fg, lane);
        }
        for (int x = tid; x < W; x += 256) {
            if (cc_is_start(wf, x)) {                                  // a run of P' is a whole run of P: components are kept whole
                const int h = cc_popcount(wg, x, cc_run_end(wf, x, nw));
                if (h) atomicAdd(hit + b * hw + parent[r * W + x], h);
            }
            if (cc_is_start(wg, x)) {
                const int h = cc_popcount(wf, x, cc_run_end(wg, x, nw));
                if (h) atomicAdd(hit + (b + B) * hw + parent[rg * W + x], h);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cc_count_kernel(int B, int H, int W, CcFilter f, const int* __restrict__ parent, const int* __restrict__ area,
                                                       const int* __restrict__ hit, u64* __restrict__ acc) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long rows = 2l * B * H;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long plane = r / H;
        const int y = (int)(r % H), is_g = plane >= B ? 1 : 0;
        u64* a = acc + (plane - (is_g ? B : 0)) * CC_ACC;
        const u64 best = a[CC_ACC_BEST];
        unsigned n_kept = 0u, n_ok = 0u, n_gone = 0u;
        for (int x0 = 0; x0 < W; x0 += 256) {
            const int x = x0 + tid;
            if (x < W && parent[r * W + x] == y * W + x) {
                const int ar = area[r * W + x], h = hit[r * W + x];
                if (is_g) {
                    n_ok += cc_overlaps(f, h, ar) ? 1u : 0u;
                } else if (cc_kept(f, ar, y * W + x, best)) {
                    ++n_kept;
                    n_ok += cc_overlaps(f, h, ar) ? 1u : 0u;
                } else {
                    ++n_gone;
                }
            }
        }
        cc_wave_add(a + 6 + is_g, n_ok, lane);
        if (!is_g) {                                                   // uniform
            cc_wave_add(a + 4, n_kept, lane);
            cc_wave_add(a + 11, n_gone, lane);
        }
    }
}

__global__ __launch_bounds__(256) void cc_finish_kernel(int B, const u64* __restrict__ acc, long long* __restrict__ ints) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B * MI_LESION_INTS) ints[i] = (long long)acc[(long)(i / MI_LESION_INTS) * CC_ACC + i % MI_LESION_INTS];
}

inline dim3 cc_grid(long n) { return dim3((unsigned)(n < CC_MAX_GRID ? n : CC_MAX_GRID)); }

// rows, merge, flatten: the three launches both entries share.
void cc_label_planes(const CcSrc& src, long planes, int H, int W, int connectivity, const CcWs& w, int* hit, int* rowcnt, hipStream_t s) {
    const dim3 grid = cc_grid(planes * H);
    hipLaunchKernelGGL(cc_rows_kernel, grid, dim3(256), 0, s, src, planes, H, W, w.bits, w.parent, w.area, hit);
    hipLaunchKernelGGL(cc_merge_kernel, grid, dim3(256), 0, s, planes, H, W, connectivity == 8 ? 1 : 0, w.bits, w.parent);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, dim3(256), 0, s, planes, H, W, w.bits, w.parent, w.area, rowcnt);
}

}  // namespace

extern "C" size_t mi_label_components_workspace(int B, int H, int W) {
    if (!cc_sizes_ok(B, H, W)) return 0;
    return cc_layout(nullptr, B, H, W, false).bytes;
}

extern "C" int mi_label_components(const uint8_t* mask, int B, int H, int W, int cls, int connectivity, int32_t* labels, int32_t* roots, int32_t* counts,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(mask && counts && workspace, "mi_label_components: null operand");
    MI_REQUIRE(labels || roots, "mi_label_components: null operand (labels and roots are both NULL)");
    MI_REQUIRE(B > 0 && H > 0 && W > 0, "mi_label_components: bad dimension (B %d, masks %d x %d)", B, H, W);
    MI_REQUIRE(cc_sizes_ok(B, H, W), "mi_label_components: B %d, masks %d x %d beyond the limits (B <= 65535, sides <= %d)", B, H, W, CC_MAX_SIDE);
    MI_REQUIRE(cls >= 0 && cls <= 255, "mi_label_components: cls %d lies outside 0..255", cls);
    MI_REQUIRE(connectivity == 4 || connectivity == 8, "mi_label_components: connectivity %d is neither 4 nor 8", connectivity);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mi_label_components: workspace must be 8-byte aligned");
    const CcWs w = cc_layout(workspace, B, H, W, false);
    if (workspace_bytes < w.bytes) return mi_set_error(MI_ENOMEM, "mi_label_components: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const CcSrc src = {mask, nullptr, B, cls};
    const long hw = (long)H * W, px_wgs = ((long)B * hw + 255) / 256;
    cc_label_planes(src, B, H, W, connectivity, w, nullptr, w.rowcnt, s);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(B), dim3(256), 0, s, H, w.rowcnt, counts);
    hipLaunchKernelGGL(cc_number_kernel, cc_grid((long)B * H), dim3(256), 0, s, (long)B, H, W, w.parent, w.rowcnt, w.area);
    hipLaunchKernelGGL(cc_write_kernel, cc_grid(px_wgs), dim3(256), 0, s, (long)B, hw, w.parent, w.area, labels, roots);
    MI_CHECK_LAUNCH("mi_label_components");
    return MI_OK;
}

extern "C" size_t mi_lesion_score_workspace(int B, int H, int W) {
    if (!cc_sizes_ok(B, H, W)) return 0;
    return cc_layout(nullptr, 2l * B, H, W, true).bytes;
}

extern "C" int mi_lesion_score(const uint8_t* pred, const int64_t* labels, int B, int H, int W, int cls, int connectivity, int min_area, int keep_largest,
                               int overlap_permille, uint8_t* filtered, int64_t* ints, void* workspace, size_t workspace_bytes, void* stream) {
    MI_REQUIRE(pred && labels && ints && workspace, "mi_lesion_score: null operand");
    MI_REQUIRE(B > 0 && H > 0 && W > 0, "mi_lesion_score: bad dimension (B %d, masks %d x %d)", B, H, W);
    MI_REQUIRE(cc_sizes_ok(B, H, W), "mi_lesion_score: B %d, masks %d x %d beyond the limits (B <= 65535, sides <= %d)", B, H, W, CC_MAX_SIDE);
    MI_REQUIRE(cls >= 0 && cls <= 255, "mi_lesion_score: cls %d lies outside 0..255", cls);
    MI_REQUIRE(connectivity == 4 || connectivity == 8, "mi_lesion_score: connectivity %d is neither 4 nor 8", connectivity);
    MI_REQUIRE(min_area >= 0, "mi_lesion_score: min_area %d is negative", min_area);
    MI_REQUIRE(keep_largest == 0 || keep_largest == 1, "mi_lesion_score: keep_largest %d is neither 0 nor 1", keep_largest);
    MI_REQUIRE(overlap_permille >= 0 && overlap_permille <= 1000, "mi_lesion_score: overlap_permille %d lies outside 0..1000", overlap_permille);
    MI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mi_lesion_score: workspace must be 8-byte aligned");
    const long planes = 2l * B;
    const CcWs w = cc_layout(workspace, planes, H, W, true);
    if (workspace_bytes < w.bytes) return mi_set_error(MI_ENOMEM, "mi_lesion_score: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    hipStream_t s = (hipStream_t)stream;
    const CcSrc src = {pred, reinterpret_cast<const long long*>(labels), B, cls};
    const CcFilter f = {min_area, keep_largest, overlap_permille};
    if (hipMemsetAsync(w.acc, 0, (size_t)B * CC_ACC * sizeof(u64), s) != hipSuccess) return mi_set_error(MI_EHIP, "mi_lesion_score: memset failed");
    cc_label_planes(src, planes, H, W, connectivity, w, w.hit, nullptr, s);
    hipLaunchKernelGGL(cc_select_kernel, cc_grid(planes * H), dim3(256), 0, s, B, H, W, f, w.parent, w.area, w.acc);
    hipLaunchKernelGGL(cc_hits_kernel, cc_grid((long)B * H), dim3(256), 0, s, B, H, W, cls, f, w.bits, w.parent, w.area, w.hit, w.acc, filtered);
    hipLaunchKernelGGL(cc_count_kernel, cc_grid(planes * H), dim3(256), 0, s, B, H, W, f, w.parent, w.area, w.hit, w.acc);
    hipLaunchKernelGGL(cc_finish_kernel, dim3((B * MI_LESION_INTS + 255) / 256), dim3(256), 0, s, B, w.acc, reinterpret_cast<long long*>(ints));
    MI_CHECK_LAUNCH("mi_lesion_score");
    return MI_OK;
}
