// wino4_input.h - the input side of wino4.hip's kernels, included as text inside a kernel's braces (see wino4_body.h for why
// text and not a device function): this thread's (tile, channel) item, its patch loads (pload) and the BN+FiLM+leaky prologue,
// zero padding and 6x6 transform B^T d B into the V image at `lv` (pprocess).  One text for wino4_kernel / wino4_splitk_kernel,
// which run it per chunk in front of their MFMA phase, and for wino4_vprep_kernel, which runs it once per (block, chunk, clip)
// and leaves the image in memory.  In scope: TC, PRO, PRE, p, tid, y0, x0, HW, in_b, sc, sh, lv.
    // ---- this thread's item: tile pt (0..31) and channel c8 (0..7) of the chunk; its 6x6 patch, top-left (gy0, gx0) ------
    const int pt = tid & 31, c8 = (tid & 255) >> 5;  // (tid < 256: see afrag)
    const int pty = pt / TC, ptx = pt % TC;
    const int gy0 = y0 + 4 * pty - 1, gx0 = x0 + 4 * ptx - 1;
    const bool left = gx0 < 0, right = gx0 + 5 >= p.W;
    unsigned vo_c[6], vo_l[6], vo_r[6], rowok = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int gy = gy0 + i;
        const int row = (PRE ? 0 : c8 * HW) + min(max(gy, 0), p.H - 1) * p.W;
        vo_c[i] = 4u * (unsigned)(row + gx0 + 1);                 // columns gx0+1 .. gx0+4: 16-byte aligned, always inside
        vo_l[i] = 4u * (unsigned)(row + (left ? 0 : gx0));        // column gx0 (clamped at the left edge)
        vo_r[i] = 4u * (unsigned)(row + (right ? p.W - 1 : gx0 + 5));
        rowok |= (gy >= 0 && gy < p.H ? 1u : 0u) << i;
    }
    const __amdgpu_buffer_rsrc_t in_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b), 0, (int)((unsigned)(PRE ? 1 : p.Cin) * (unsigned)HW * 4u), 0x00020000);
    const bool edge = left || right || rowok != 0x3fu;  // this item's patch reaches into the zero padding
    float4 pc[6];
    float pl[6], pr[6], ps = 1.f, ph = 0.f;
    const unsigned tvo = (unsigned)c8 * 4u;  // this item's entry of a per-channel table, within the chunk
    const auto tab_rsrc = [&](const float* t, int n) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(t), 0, n * 4, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t sc_rsrc = tab_rsrc(PRO ? sc : p.in, p.Cin), sh_rsrc = tab_rsrc(PRO ? sh : p.in, p.Cin);
    const __amdgpu_buffer_rsrc_t pw_rsrc = tab_rsrc(PRE ? p.pre_w : p.in, 32), pb_rsrc = tab_rsrc(PRE ? p.pre_b : p.in, 32);
    auto pload = [&](int ch) {
        const unsigned soff = PRE ? 0u : (unsigned)(ch * KC * HW) * 4u;
        if (!PRE || ch == 0)  // PRE: every channel is an affine function of the one x0 patch, loaded once
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            pc[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, (int)vo_c[i], (int)soff, 0));
            pl[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, (int)vo_l[i], (int)soff, 0));
            pr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(in_rsrc, (int)vo_r[i], (int)soff, 0));
        }
        // The table reads are buffer loads as well (one vector-memory instruction each, by construction): the conv kernels'
        // wait_vmcnt<NLOAD> (wino4_body.h) counts them, and a plain C++ load could be merged, hoisted or scalarised by the compiler
        // behind the count's back.  (wino4_vprep_kernel has no such wait: the compiler's own vmcnt orders its loads.)
        const unsigned toff = (unsigned)(ch * KC) * 4u;
        if (PRO) {
            ps = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sc_rsrc, (int)tvo, (int)toff, 0));
            ph = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sh_rsrc, (int)tvo, (int)toff, 0));
        }
        if (PRE) {  // leaky(bn(pre_w x0 + pre_b) + beta) = leaky(x0 * (pre_w s) + (pre_b s + h))
            const float pw = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pw_rsrc, (int)tvo, (int)toff, 0));
            const float pb = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(pb_rsrc, (int)tvo, (int)toff, 0));
            ph = fmaf(pb, ps, ph);
            ps = pw * ps;
        }
    };
    constexpr int NLOAD = (PRE ? 0 : 6 * 3) + (PRO ? 2 : 0) + (PRE ? 2 : 0);  // vector-memory operations of one pload (chunks >= 1)
    // V destination of this item: row (xi, kq = c8 % 4), column tile ^ swizzle, k-step c8 / 4; xi stride = 4 * 64 floats
    float* vdst = lv + ((c8 & 3) * 32 + (pt ^ ((c8 & 1) << 4))) * 2 + (c8 >> 2);
    auto pprocess = [&]() {
        float d[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float v[6] = {pl[i], pc[i].x, pc[i].y, pc[i].z, pc[i].w, pr[i]};
#pragma unroll
            for (int jx = 0; jx < 6; ++jx) d[i][jx] = PRO ? leaky(fmaf(v[jx], ps, ph)) : v[jx];
        }
        // zero padding comes AFTER the activation (resunet.py:150, conv padding) and touches only the outer ring of the patch
        // (row 0 / 5, column 0 / 5) of the items at the image border: wave-uniform branch, skipped by interior waves
        if (__builtin_amdgcn_ballot_w64(edge) != 0) {
            const bool r0 = (rowok & 1u) != 0, r5 = (rowok & 32u) != 0;
#pragma unroll
            for (int jx = 0; jx < 6; ++jx) {
                d[0][jx] = r0 ? d[0][jx] : 0.f;
                d[5][jx] = r5 ? d[5][jx] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                d[i][0] = left ? 0.f : d[i][0];
                d[i][5] = right ? 0.f : d[i][5];
            }
        }
        float tt[6][6];  // B^T d: columns
#pragma unroll
        for (int jx = 0; jx < 6; ++jx) {
            const float col[6] = {d[0][jx], d[1][jx], d[2][jx], d[3][jx], d[4][jx], d[5][jx]};
            float r[6];
            bt6(col, r);
#pragma unroll
            for (int i = 0; i < 6; ++i) tt[i][jx] = r[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {  // (B^T d) B: rows
            float r[6];
            bt6(tt[i], r);
#pragma unroll
            for (int jx = 0; jx < 6; ++jx) vdst[(i * 6 + jx) * 256] = r[jx];
        }
    };
