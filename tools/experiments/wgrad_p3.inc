// wgrad_p3_kernel: the 8-wave fused-row 3x3 weight gradient (ping-pong main loop, one workgroup per CU) - an opt-in kernel that does not win
// (DESIGN.md section 8).  Not a translation unit: csrc/igemm_tn.hip includes this file inside its anonymous namespace under MI_EXPERIMENTS
// (tools/experiments/build.sh), behind the P3_* constants, WgradP3Params and the helpers it uses (tr_read_lds, glds16_tn, wg_decode_tile, slab_store).
__global__ __launch_bounds__(512, 1) void wgrad_p3_kernel(WgradP3Params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wq = wave & 3;
    const WgDecode wg = wg_decode_tile<TO, TI>(blockIdx.x, p.o_tiles * p.i_tiles * 3 * p.S, p.o_tiles, p.i_tiles, 3);
    const int ky = wg.mid, split = wg.split, o0 = wg.o0, i0 = wg.i0;
    const long q_begin = (p.dbg & 16) ? 0 : (long)split * p.slabs_per_split * P3_KS;      // dbg 16: every split streams the same (L2-hot) rows
    long left = (p.Q - q_begin + P3_KS - 1) / P3_KS;
    const int ns = (int)(left < 0 ? 0 : (left < p.slabs_per_split ? left : p.slabs_per_split));
    // ---- DMA roles.  lane -> (row within the piece, physical 16-B chunk); it fetches logical chunk physical ^ ((row & 7) << 1).
    const int prow = lane >> 4, pch = lane & 15;
    // zero rows (pad slots, rows outside the image, tile tails): 16 lanes read the 256-B zero page as one contiguous row
    const char* zero = reinterpret_cast<const char*>(g_zero_page_tn) + pch * 16;
    // A wave stages a SPAN of consecutive padded coordinates per slab (16 dy rows or 20 window rows): piece j = rows 4j .. 4j+3.
    // The span's first row is wave-uniform, so its coordinates (q, padded column wp, image row h, pixel index pix) live in
    // scalar registers and advance with scalar arithmetic: 64 coordinates = n0 whole image rows + r0 columns (+ one carry).
    // Fast path (3 of 4 slabs at W = 97): the whole span lies inside the real columns of one valid image row -> the rows are
    // consecutive pixels, address = scalar base + a per-lane constant (2 vector ops per piece).  Otherwise every lane derives
    // its row's coordinates from the scalars (one carry at most: the plan requires span <= WP).
    constexpr int NPMAX = P3_NPX;
    const int np = grp == 0 ? P3_NPY : P3_NPX;
    const int span = np * 4;
    const int dh = grp == 0 ? 0 : (ky - 1) * p.d;
    const int n0 = P3_KS / p.WP, r0 = P3_KS - n0 * p.WP;
    const int pix_step = n0 * p.W + r0;                 // minus 2d when the column wraps into the next image row
    const int span0 = grp == 0 ? wq * (P3_NPY * 4) : wq * (P3_NPX * 4);
    int s_q = (int)(q_begin + span0 - (grp == 0 ? 0 : p.d));                 // may be < 0 (first window rows of split 0)
    int s_wp, s_h, s_pix;
    {
        const long qs = (long)s_q + p.WP;                                     // >= 0 (d <= WP)
        const int bh = (int)(qs / p.WP) - 1;
        s_wp = (int)(qs % p.WP);
        s_h = bh < 0 ? p.H - 1 : bh % p.H;                                    // row -1 precedes row 0 of image 0
        s_pix = (bh + dh) * p.W + s_wp - p.d;
    }
    // the lane's channel chunk depends on (row & 7), i.e. on the parity of the piece: two per-lane constants
    const __bf16* opnd = grp == 0 ? p.dY : p.X;
    const int c0 = grp == 0 ? o0 : i0, cmax = grp == 0 ? p.O : p.I;
    const unsigned row_bytes = (unsigned)cmax * 2u;
    const int lch_e = pch ^ (((span0 + prow) & 7) << 1), lch_o = pch ^ (((span0 + prow + 4) & 7) << 1);
    const bool ok_e = c0 + lch_e * 8 < cmax, ok_o = c0 + lch_o * 8 < cmax;
    const unsigned off_e = prow * row_bytes + (c0 + lch_e * 8) * 2, off_o = prow * row_bytes + (c0 + lch_o * 8) * 2;
    const char* opnd_b = reinterpret_cast<const char*>(opnd);
    const int Qi = (int)p.Q;
    int ld_s = 0;
    auto stage_next = [&]() {
        char* dst = smem + (ld_s & 3) * P3_SLAB + (grp == 0 ? wq * (P3_NPY * 1024) : P3_DY_BYTES + wq * (P3_NPX * 1024));
        const bool fast = s_q >= 0 && s_q + span <= Qi && s_wp >= p.d && s_wp + span <= p.W + p.d && (unsigned)(s_h + dh) < (unsigned)p.H;
        if (fast) {
            const char* P = opnd_b + (unsigned long)(unsigned)s_pix * row_bytes;              // scalar
#pragma unroll
            for (int j = 0; j < NPMAX; ++j)
                if (j < np) {
                    const char* src = P + (j * 4 * row_bytes + ((j & 1) ? off_o : off_e));
                    glds16_tn(((j & 1) ? ok_o : ok_e) ? src : zero, dst + j * 1024);
                }
        } else {
#pragma unroll
            for (int j = 0; j < NPMAX; ++j)
                if (j < np) {
                    const int r = j * 4 + prow;
                    int wp = s_wp + r;
                    const bool c = wp >= p.WP;
                    wp -= c ? p.WP : 0;
                    int h = s_h + (c ? 1 : 0);
                    h = h >= p.H ? h - p.H : h;
                    const int pix = s_pix + r - (c ? 2 * p.d : 0);
                    const bool ok = ((j & 1) ? ok_o : ok_e) && (unsigned)(s_q + r) < (unsigned)Qi && (unsigned)(wp - p.d) < (unsigned)p.W &&
                                    (unsigned)(h + dh) < (unsigned)p.H;
                    const char* src = opnd_b + (unsigned long)(unsigned)(ok ? pix : 0) * row_bytes + (((j & 1) ? off_o : off_e) - prow * row_bytes);
                    glds16_tn(ok ? src : zero, dst + j * 1024);
                }
        }
        // the span's first row in the next slab (scalar)
        s_q += P3_KS;
        s_wp += r0;
        const int c = s_wp >= p.WP ? 1 : 0;
        s_wp -= c ? p.WP : 0;
        s_h += n0 + c;
        s_h = s_h >= p.H ? s_h - p.H : s_h;
        s_pix += pix_step - (c ? 2 * p.d : 0);
        ++ld_s;
    };

    // ---- compute roles: wave (wi, wo) owns i in [wi*32, +32) x o in [wo*64, +64) for the three taps kx
    const int wi = wq, wo = grp;
    f32x4 acc[3][2][4];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[kx][a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, q4 = (lane & 15) >> 2, pc = lane & 3;
    const int rk0 = g * 4 + q4;
    const int y_off = rk0 * ROWB + (pc & 1) * 8, y_sw = (rk0 & 7) << 1;
    int x_off[3], x_sw[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int rk = rk0 + kx * p.d;
        x_off[kx] = P3_DY_BYTES + rk * ROWB + (pc & 1) * 8;
        x_sw[kx] = (rk & 7) << 1;
    }
    union Frag { bf16x8 v; s16x4 h[2]; };
    Frag yf[2][4], xf[2][3][2];
    const unsigned lds0 = lds_address(smem);
    auto read_frags = [&](int s) {
        unsigned sb = lds0 + (s & 3) * P3_SLAB;
        asm volatile("" : "+v"(sb));          // opaque: keeps the 10 fragment offsets, not 40 precomputed per-slot addresses, in registers
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned base = sb + y_off + ((((wo * 4 + b) * 2 + (pc >> 1)) ^ y_sw) << 4);
            yf[0][b].h[0] = tr_read_lds<0>(base);
            yf[0][b].h[1] = tr_read_lds<16 * ROWB>(base);
            yf[1][b].h[0] = tr_read_lds<32 * ROWB>(base);
            yf[1][b].h[1] = tr_read_lds<48 * ROWB>(base);
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const unsigned base = sb + x_off[kx] + ((((wi * 2 + a) * 2 + (pc >> 1)) ^ x_sw[kx]) << 4);
                xf[0][kx][a].h[0] = tr_read_lds<0>(base);
                xf[0][kx][a].h[1] = tr_read_lds<16 * ROWB>(base);
                xf[1][kx][a].h[0] = tr_read_lds<32 * ROWB>(base);
                xf[1][kx][a].h[1] = tr_read_lds<48 * ROWB>(base);
            }
    };
    auto mfma_half = [&](int ks) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[kx][a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[ks][kx][a].v, yf[ks][b].v, acc[kx][a][b], 0, 0, 0);
    };

    // ---- main loop (interval scheme of igemm_pp.hip) ----------------------------------------------------------------------------
    for (int s = 0; s < 3 && s < ns; ++s) stage_next();
    if (ns >= 3) {
        if (grp == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P3_NPY) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P3_NPX) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();
    const int dbg = p.dbg;
    for (int s = 0; s < ns; ++s) {
        if (s + 3 < ns && !(dbg & 1)) stage_next();
        if (!(dbg & 2) || s == 0) read_frags(s);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (grp == 1) {
            if (s + 3 < ns) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P3_NPX) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_setprio(1);
        if (!(dbg & 4)) {
            mfma_half(0);
            mfma_half(1);
        }
        __builtin_amdgcn_s_setprio(0);
        if (grp == 0) {
            if (s + 3 < ns) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P3_NPY) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();

    // ---- partial planes: slab[split][ky*3+kx][o][i], i fastest; lane owns o = column, i .. i+3 = rows
    if (dbg & 8) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) asm volatile("" ::"v"(acc[kx][a][b]));
        return;
    }
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
        slab_store(p.slab + ((long)(split * 9 + ky * 3 + kx) * p.O) * p.I, p.I, p.O, p.I, o0 + wo * 64, i0 + wi * 32, lane, acc[kx]);
}
