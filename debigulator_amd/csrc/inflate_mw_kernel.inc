// inflate_mw_kernel.inc -- the same inflate as inflate_kernel.inc, but ONE STREAM PER WORKGROUP
// OF NW WAVEFRONTS, for batches of few large streams (big PNG images, long gzip members) that
// cannot fill the chip with one wavefront per stream.
//
// Everything per-lane is shared with the single-wavefront kernel (tables, lenient scan,
// half-segment decode, far copy, pending-bitmap resolve).  What changes is the width: the
// input window is 64*NW segments, the LDS output tile NW*4 KiB, and whatever the single
// wavefront exchanged by shuffles (predecessor's end, prefix sums, error votes) crosses
// wavefronts through a small LDS exchange area between workgroup barriers.  The ordered
// near-match resolve is spread over the wavefronts too (resolve_matches in inflate_kernel.inc).
//
// Included after inflate_kernel.inc by debig_hip.hip (hipcc) and the CPU emulator build.

template <int NW> struct MwExchange {
    uint32_t end[64 * NW];        /* pass 1: lenient end of every segment            */
    uint32_t start[64 * NW];      /* converged start                                 */
    uint32_t mid_lp[64 * NW];
    uint32_t nsym[64 * NW];
    uint32_t mid_nsym[64 * NW];
    uint32_t mid_nbytes[64 * NW];
    int64_t o[64 * NW + 1];       /* output offset of every segment                  */
    unsigned long long cont[NW];  /* per wavefront: lanes whose strict flag is CONT   */
    uint32_t vote[NW];            /* per wavefront boolean                            */
    uint32_t wtot[NW];            /* per wavefront output byte total                  */
    uint32_t err_code[NW];        /* pass 2: first failing lane of the wavefront      */
    int64_t err_pos[NW];
    int64_t min_oc[NW];
    uint32_t wflag, wstatus, wend; /* of the last used segment                        */
    uint32_t build_ok;
};

#ifndef DEBIG_MW_PRIO
#define DEBIG_MW_PRIO 1
#endif
#ifndef DEBIG_MW_PRIO_BYTES
#define DEBIG_MW_PRIO_BYTES (512u << 10)
#endif
template <int NW>
__global__ void __launch_bounds__(64 * NW)
debig_inflate_mw_kernel(const uint8_t *__restrict__ in_arena, uint8_t *__restrict__ out_arena,
                        const debig_stream *__restrict__ streams, debig_result *results,
                        uint32_t n_streams, const uint32_t *__restrict__ fixed_tabs, uint32_t stream_class)
{
    __shared__ WaveLdsT<NW> S;
    __shared__ MwExchange<NW> X;
    constexpr uint32_t NTH = 64u * NW;
    constexpr uint32_t TILE = DEBIG_T * NW;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;

    for (uint32_t sid = blockIdx.x; sid < n_streams; sid += gridDim.x) {
        const debig_stream st = streams[sid];
        if (!stream_in_class(st, stream_class)) continue; /* workgroup-uniform */
        if (stream_class == 3u) { /* DEBIG_CLASS_RETRY: only what the scan / LZ77 / chunk kernels handed back */
            const uint32_t handed = results[sid].status;
            __syncthreads(); /* every thread has read it before thread 0 writes the new result */
            if (handed != 11u /* DEBIG_E_RETRY */) continue;
        }
        const uint8_t *in = in_arena + st.in_off;
        const uint64_t in_len = st.in_len;
#if !defined(DEBIG_EMU) && DEBIG_MW_PRIO
        // a long stream sets the run time of a mixed batch (config 3: 28 ms for the 1 MB streams alone,
        // 40 ms with the small ones beside them): its wavefronts go first at the SIMD's arbiter, the
        // short streams fill the gaps
        if (in_len >= DEBIG_MW_PRIO_BYTES) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(0);
#endif
        OutState O;
        O.out = out_arena + st.out_off;
        O.out_cap = st.out_cap;
        O.outpos = 0;
        O.lds_from = 0;
        O.tile_base = align_anchor(O.out, 0);

        PROF_DECL
        uint32_t status = DEBIG_OK, good = 0, final_set = 0;
        uint32_t n_blocks = 0, n_windows = 0, n_rounds = 0;
        int64_t end_bits = 0; /* debig_result.in_end_bits */
        int tables = 0;
        int64_t staged_base = 0; /* stage_window_cached state */
        int staged_valid = 0;
        int short_mode = 0; /* the previous symbol window ended inside the first segment */

        if (!(st.flags & DEBIG_STREAM_NO_REF_GATES)) {
            if (st.out_cap < in_len) status = DEBIG_E_GATE_RECIPIENT_SMALL;
            else if (in_len < 5) status = DEBIG_E_GATE_INPUT_SHORT;
        }
        if (status == DEBIG_OK) {
            final_set = 1;
            for (uint32_t k = tid; k < TILE / 32 + 16; k += NTH) { S.bitmap[k] = 0; S.farmap[k] = 0; }
            for (uint32_t k = tid; k < (TILE + DEBIG_TSLACK) / 32 + 2; k += NTH) S.pend[k] = 0;
            if (tid == 0) S.internal_err = 0;
            __syncthreads();

            int64_t bitpos = 0;
            int more = 1;
            while (more && status == DEBIG_OK) {
                // ---- block header: every thread runs the same reader on the staged bytes
                PROF_BEGIN();
                int64_t wbase = stage_window_cached(S, in, in_len, bitpos >> 3, DEBIG_HEADER_NEED, 0, staged_base, staged_valid);
                int64_t org = 8 * wbase;
                BitRd hb;
                br_init(hb, S, bitpos, org);
                br_ensure(hb, S);
                uint32_t bfinal = br_take(hb, 1);
                uint32_t btype = br_take(hb, 2);
                if (bfinal) more = 0;
                n_blocks++;
                if (btype == 3) {
                    bitpos = hb.pos;
                    continue;
                }
                if (btype == 0) {
                    int64_t p = (hb.pos + 7) & ~(int64_t)7;
                    br_init(hb, S, p, org);
                    br_ensure(hb, S);
                    uint32_t len = br_take(hb, 16);
                    br_ensure(hb, S);
                    uint32_t nlen = br_take(hb, 16);
                    if ((len ^ nlen) != 0xffffu) { status = DEBIG_E_STORED_NLEN; break; }
                    if ((uint64_t)O.outpos + len > O.out_cap) { status = DEBIG_E_OUTPUT_FULL; break; }
                    flush_all(S, O);
                    stored_copy<NW>(in, in_len, hb.pos >> 3, O.out + O.outpos, len);
                    wave_mem_fence();
                    __syncthreads();
                    O.outpos += len;
                    O.lds_from = O.outpos;
                    O.tile_base = align_anchor(O.out, O.outpos);
                    bitpos = hb.pos + 8 * (int64_t)len;
                    continue;
                }

                // ---- Huffman block: tables (built by wavefront 0, shared by all)
                const int fixed = (btype == 1);
                const int need_p2 = st.p2_on && (O.outpos > st.p2_s0);
                if (fixed) {
                    if (tables != 1) {
                        __syncthreads();
                        const uint32_t *src = fixed_tabs;
                        uint32_t *dstw = reinterpret_cast<uint32_t *>(&S.t);
                        for (uint32_t k = tid; k < sizeof(S.t) / 4; k += NTH) dstw[k] = src[k];
                        __syncthreads();
                        tables = 1;
                    }
                } else {
                    uint32_t hlit = br_take(hb, 5) + 257u;
                    uint32_t hdist = br_take(hb, 5) + 1u;
                    uint32_t hclen = br_take(hb, 4) + 4u;
                    __syncthreads(); /* nobody still decodes with the previous tables */
                    if (tid < 19) S.lens[tid] = 0;
                    __syncthreads();
                    read_cl_lens(S, hb, org, hclen);
                    __syncthreads();
                    if (tid < 19) S.cl_len[tid] = S.lens[tid];
                    tables = 2;
                    if (wave == 0) {
                        int ok = build_code(S, CODE_CL, S.lens, 19, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES));
                        if (ok && need_p2 && lane < 19) {
                            uint32_t l = S.cl_len[lane];
                            uint32_t used = l != 0, code = 1234543u;
                            if (used) {
                                uint32_t rank = 0;
                                for (uint32_t j = 0; j < lane; j++) rank += (S.cl_len[j] == l);
                                code = (uint32_t)S.t.first[CODE_CL][l] + rank;
                            }
                            S.cl_code[lane] = code;
                            S.cl_used[lane] = used;
                        }
                        if (lane == 0) X.build_ok = (uint32_t)ok;
                    }
                    __syncthreads();
                    if (!X.build_ok) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                    // code lengths of the two alphabets, uniform over the whole workgroup
                    const uint32_t total = hlit + hdist;
                    const int bad = decode_code_lengths(S, hb, org, total);
                    if (bad) { status = DEBIG_E_NO_CODE; break; }
                    __syncthreads();
                    if (wave == 0) {
                        int ok = build_code(S, CODE_LIT, S.lens, hlit, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES));
                        if (ok) ok = build_code(S, CODE_DIST, S.lens + hlit, hdist, (int)(st.flags & DEBIG_STREAM_NO_REF_GATES));
                        if (lane == 0) X.build_ok = (uint32_t)ok;
                    }
                    __syncthreads();
                    if (!X.build_ok) { status = DEBIG_E_BAD_CODE_LENGTHS; break; }
                }
                if (need_p2) {
                    flush_all(S, O);
                    int64_t end = O.outpos < (int64_t)st.p2_est ? O.outpos : (int64_t)st.p2_est;
                    int64_t s_lo = st.p2_s0 > 0 ? st.p2_s0 : 0;
                    uint32_t nent = fixed ? 288u : 19u;
                    for (int64_t s = s_lo + tid; s < end; s += NTH) {
                        uint64_t t = (uint64_t)(s - st.p2_s0);
                        uint64_t e = t >> 4;
                        uint32_t k = (uint32_t)(t & 15u);
                        if (e >= nent) { O.out[s] = 0; continue; }
                        if (k >= 14) continue;
                        uint32_t code, used, l;
                        if (fixed) {
                            uint32_t ei = (uint32_t)e;
                            used = 1;
                            if (ei < 144) { l = 8; code = 48 + ei; }
                            else if (ei < 256) { l = 9; code = 400 + (ei - 144); }
                            else if (ei < 280) { l = 7; code = ei - 256; }
                            else { l = 8; code = 192 + (ei - 280); }
                        } else {
                            code = S.cl_code[e]; used = S.cl_used[e]; l = S.cl_len[e];
                        }
                        uint32_t word = k < 4 ? code : k < 8 ? (uint32_t)e : k < 12 ? used : l;
                        O.out[s] = (uint8_t)(word >> (8 * (k & 3u)));
                    }
                    wave_mem_fence();
                    __syncthreads();
                }
                bitpos = hb.pos;
                PROF_END(5);

                // ---- symbol windows of 64*NW segments
                int block_done = 0;
                while (!block_done && status == DEBIG_OK) {
                    n_windows++;
                    SegInfo si = seg_info_empty();
                    uint32_t start = 0, first_term = NTH;
                    int probe_hit = 0;
                    if (short_mode) {
                        // short blocks: thread 0 alone decodes strictly from the true position
                        // (see debig_inflate_kernel); the verdict crosses wavefronts through LDS
                        PROF_BEGIN();
                        wbase = stage_window_cached(S, in, in_len, bitpos >> 3, DEBIG_PROBE_NEED, 0, staged_base, staged_valid);
                        org = 8 * wbase;
                        PROF_END(0);
                        PROF_BEGIN();
                        int64_t ptl = 8 * ((int64_t)in_len - 1) - org;
                        const int32_t ptail = ptl < -1 ? -1 : (ptl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)ptl);
                        start = (uint32_t)(bitpos - org);
                        if (tid == 0) {
                            si = scan_segment<true>(S, start, start + SegCfg<NW>::BITS, ptail);
                            X.wflag = si.flag;
                        }
                        n_rounds++;
                        __syncthreads();
                        probe_hit = X.wflag != FL_CONT;
                        __syncthreads(); /* X.wflag is rewritten below */
                        if (probe_hit) first_term = 0;
                        else { short_mode = 0; si = seg_info_empty(); }
                        PROF_END(1);
                    }
                    if (!probe_hit) {
                    PROF_BEGIN();
                    wbase = stage_window_cached(S, in, in_len, bitpos >> 3, SegCfg<NW>::WIN + 16u, 1, staged_base, staged_valid);
                    PROF_END(0);
                    PROF_BEGIN();
                    org = 8 * wbase;
                    const uint32_t seg_lo = tid * SegCfg<NW>::BITS;
                    const uint32_t seg_end = seg_lo + SegCfg<NW>::BITS;
                    start = (tid == 0) ? (uint32_t)(bitpos - org) : seg_lo;
                    int64_t tl = 8 * ((int64_t)in_len - 1) - org;
                    const int32_t tail_l = tl < -1 ? -1 : (tl > 0x7ffffff0 ? 0x7ffffff0 : (int32_t)tl);
                    int dirty = 1;
                    si.end = start; si.strict_end = start; si.nbytes = 0; si.nsym = 0;
                    si.flag = FL_CONT; si.status = 0; si.mid_lp = start; si.mid_nbytes = 0; si.mid_nsym = 0;
                    first_term = NTH;
                    const uint32_t npos = fixed ? DEBIG_POS_ROUNDS_FIXED : DEBIG_POS_ROUNDS_DYNAMIC;
                    for (uint32_t round = 0; round < 64 * NW + 6 + npos; round++) {
                        if (round < npos) {
                            // round 0 of narrow segments starts a segment early (SegCfg::LEAD_BITS)
                            const uint32_t from = (round == 0 && tid > 0) ? seg_lo - SegCfg<NW>::LEAD_BITS : start;
                            if (dirty) si.end = scan_positions(S, from, seg_end);
                        }
                        else if (dirty) si = scan_segment(S, start, seg_end, tail_l);
                        dirty = round == npos - 1;
                        n_rounds++;
                        X.end[tid] = si.end;
                        unsigned long long cb = __ballot(si.flag == FL_CONT);
                        if (lane == 0) X.cont[wave] = cb;
                        __syncthreads();
                        first_term = NTH;
                        for (int w = NW - 1; w >= 0; w--) {
                            unsigned long long c = X.cont[w];
                            if (~c != 0ull) first_term = 64u * (uint32_t)w + (uint32_t)(__ffsll(~c) - 1);
                        }
                        if (tid > 0) {
                            uint32_t prev_end = X.end[tid - 1];
                            if (start != prev_end) {
                                start = prev_end;
                                dirty = 1;
                            }
                        }
                        int v = __any(dirty && tid <= first_term);
                        if (lane == 0) X.vote[wave] = (uint32_t)v;
                        __syncthreads();
                        uint32_t anyv = 0;
                        for (int w = 0; w < NW; w++) anyv |= X.vote[w];
                        if (round >= npos && !anyv) break;
                        __syncthreads(); /* X.end / X.vote are rewritten next round */
                    }
                    PROF_END(1);
                    short_mode = first_term == 0;
                    } /* !probe_hit */
                    const uint32_t last = first_term < NTH ? first_term : NTH - 1;
                    const int used = tid <= last;
                    // segment data for pass 2 + offsets by prefix sum across the workgroup
                    uint32_t nbytes = used ? si.nbytes : 0u;
                    uint32_t wsum;
                    uint32_t pre = wave_excl_scan_u32(nbytes, &wsum);
                    __syncthreads();
                    if (lane == 0) X.wtot[wave] = wsum;
                    if (tid == last) { X.wflag = si.flag; X.wstatus = si.status; X.wend = si.strict_end; }
                    __syncthreads();
                    uint32_t woff = 0, wtotal = 0;
                    for (uint32_t w = 0; w < (uint32_t)NW; w++) {
                        if (w < wave) woff += X.wtot[w];
                        wtotal += X.wtot[w];
                    }
                    const uint32_t wflag = X.wflag, wstatus = X.wstatus;
                    const int64_t wend = org + (int64_t)X.wend;
                    const int64_t w_out0 = O.outpos;
                    const int64_t w_end = w_out0 + (int64_t)wtotal;
                    X.start[tid] = start;
                    X.mid_lp[tid] = si.mid_lp;
                    X.nsym[tid] = used ? si.nsym : 0u;
                    X.mid_nsym[tid] = used ? si.mid_nsym : 0u;
                    X.mid_nbytes[tid] = used ? si.mid_nbytes : 0u;
                    X.o[tid] = w_out0 + (int64_t)woff + (int64_t)pre;
                    if (tid == 0) X.o[NTH] = w_end;
                    __syncthreads();

                    uint32_t lane_err = 0;
                    int64_t lane_err_pos = 0;
                    for (uint32_t batch = 0; batch < 2 && status == DEBIG_OK; batch++) {
                        // lane j of the workgroup <-> half (j & 1) of segment 32*NW*batch + j/2
                        const uint32_t sl = 32u * NW * batch + (tid >> 1);
                        const uint32_t half = tid & 1u;
                        int64_t w_out1 = batch == 0 ? X.o[32u * NW] : w_end;
                        int64_t oc = X.o[sl] + (half ? (int64_t)X.mid_nbytes[sl] : 0);
                        uint32_t remaining = half ? X.nsym[sl] - X.mid_nsym[sl] : X.mid_nsym[sl];
                        uint32_t lp = half ? X.mid_lp[sl] : X.start[sl];
                        for (;;) {
                            const int64_t lim = O.tile_base + TILE;
                            PROF_BEGIN();
                            {
                                uint32_t rel = (uint32_t)(oc - O.tile_base);
                                const int64_t room = (int64_t)O.out_cap - O.tile_base;
                                const uint32_t cap_rel = room > 0x7fffffff ? 0x7fffffffu : (room < 0 ? 0u : (uint32_t)room);
                                const int32_t tb32 = O.tile_base > 70000 ? 70000 : (int32_t)O.tile_base;
                                const uint32_t lds_rel = (uint32_t)(O.lds_from - O.tile_base);
                                const int64_t rel_lim64 = lim - O.tile_base;
                                const uint32_t rel_lim = (oc - O.tile_base) >= rel_lim64 ? 0u : (uint32_t)rel_lim64;
                                const uint32_t lm = S.t.mask[CODE_LIT], dm = S.t.mask[CODE_DIST];
                                while (remaining && rel < rel_lim) {
                                    Win64 wb = win64(S, lp);
                                    uint32_t e = S.t.lit_tab[wb.lo & lm];
                                    if (ENT_LEN(e) == 0) e = huff_slow(wb.lo, S, CODE_LIT, e);
                                    const uint32_t l = ENT_LEN(e), nx = ENT_EXTRA(e), n1 = l + nx;
                                    const uint32_t val = ENT_VAL(e) + ((wb.lo >> l) & ((1u << nx) - 1u));
                                    const uint32_t is_len = ENT_KIND(e) == 1u;
                                    const uint32_t bits2 = funnel32(wb.hi, wb.lo, n1);
                                    uint32_t de = S.t.dist_tab[bits2 & dm];
                                    if (is_len && ENT_LEN(de) == 0) de = huff_slow(bits2, S, CODE_DIST, de);
                                    const uint32_t ld = ENT_LEN(de), dx = ENT_EXTRA(de);
                                    const uint32_t dist = ENT_VAL(de) + ((bits2 >> ld) & ((1u << dx) - 1u));
                                    const uint32_t outlen = is_len ? val : 1u;
                                    remaining--;
                                    const uint32_t too_far = is_len & (uint32_t)((int32_t)dist > tb32 + (int32_t)rel);
                                    const uint32_t full = (uint32_t)(rel + outlen > cap_rel);
                                    if (too_far | full) {
                                        lane_err = too_far ? (uint32_t)DEBIG_E_DIST_TOO_FAR : (uint32_t)DEBIG_E_OUTPUT_FULL;
                                        lane_err_pos = O.tile_base + (int64_t)rel;
                                        remaining = 0;
                                        break;
                                    }
                                    S.tile[rel] = (uint8_t)(is_len ? val - 3u : val);
                                    if (is_len) {
                                        S.tile[rel + 1] = (uint8_t)((dist - 1u) & 0xffu);
                                        S.tile[rel + 2] = (uint8_t)((dist - 1u) >> 8);
                                        uint32_t *map = ((int32_t)(rel + val) - (int32_t)dist <= (int32_t)lds_rel) ? S.farmap : S.bitmap;
                                        atomicOr(&map[rel >> 5], 1u << (rel & 31u));
                                    }
                                    lp += n1 + (is_len ? ld + dx : 0u);
                                    rel += outlen;
                                }
                                if ((oc - O.tile_base) < rel_lim64) oc = O.tile_base + (int64_t)rel;
                            }
                            PROF_END(2);
                            // error vote: the first failing work item in stream order
                            PROF_BEGIN();
                            {
                                unsigned long long em = __ballot(lane_err != 0);
                                int el = em ? __ffsll(em) - 1 : 0;
                                uint32_t es = __shfl(lane_err, el);
                                int64_t ep = __shfl(lane_err_pos, el);
                                if (lane == 0) { X.err_code[wave] = em ? es : 0u; X.err_pos[wave] = ep; }
                            }
                            // smallest write cursor among the items that still have work
                            {
                                int64_t c = remaining ? oc : w_out1;
                                for (uint32_t d = 32; d >= 1; d >>= 1) {
                                    int64_t o2 = __shfl_xor(c, (int)d);
                                    c = o2 < c ? o2 : c;
                                }
                                int v = __any(remaining != 0);
                                if (lane == 0) { X.min_oc[wave] = c; X.vote[wave] = (uint32_t)v; }
                            }
                            __syncthreads();
                            uint32_t es = 0;
                            int64_t ep = 0;
                            for (int w = NW - 1; w >= 0; w--)
                                if (X.err_code[w]) { es = X.err_code[w]; ep = X.err_pos[w]; }
                            int64_t min_oc = w_out1;
                            uint32_t any_rem = 0;
                            for (int w = 0; w < NW; w++) {
                                if (X.min_oc[w] < min_oc) min_oc = X.min_oc[w];
                                any_rem |= X.vote[w];
                            }
                            if (es) {
                                if (status == DEBIG_OK) { status = es; w_out1 = ep; }
                                remaining = 0;
                            }
                            PROF_END(5);
                            const int64_t upto = w_out1 < lim ? w_out1 : lim;
                            const uint32_t from_rel = (uint32_t)(O.outpos - O.tile_base);
                            const uint32_t to_rel = (uint32_t)(upto - O.tile_base);
                            PROF_BEGIN();
                            far_copy(S, O, from_rel, to_rel);
                            __syncthreads();
                            PROF_END(7);
                            PROF_BEGIN();
                            if (resolve_matches(S, O, from_rel, to_rel,
                                                    (st.flags & DEBIG_STREAM_FAULT_INJECT_IDLE) ? 0u : DEBIG_RESOLVE_IDLE_BOUND)) {
                                // a wavefront gave up waiting for match sources (never expected):
                                // the range holds unresolved descriptors -- fail, claim nothing of it
                                if (status == DEBIG_OK) status = DEBIG_E_INTERNAL;
                                for (uint32_t k = tid; k < TILE / 32 + 16; k += NTH) { S.bitmap[k] = 0; S.farmap[k] = 0; }
                                __syncthreads();
                                break;
                            }
                            PROF_END(3);
                            if (status != DEBIG_OK) {
                                for (uint32_t k = tid; k < TILE / 32 + 16; k += NTH) { S.bitmap[k] = 0; S.farmap[k] = 0; }
                                __syncthreads();
                                O.outpos = upto;
                                break;
                            }
                            if (w_out1 >= lim) {
                                const int64_t carry_end = min_oc > lim ? min_oc : lim;
                                PROF_BEGIN();
                                flush_range(S, O, O.lds_from, lim);
                                PROF_END(4);
                                const uint32_t carry = (uint32_t)(carry_end - lim);
                                uint8_t cv[5];
DEV_UNROLL
                                for (uint32_t it = 0; it < 5; it++) {
                                    uint32_t k = it * 64u + tid;
                                    if (tid < 64 && k < carry) cv[it] = S.tile[TILE + k];
                                }
                                __syncthreads();
DEV_UNROLL
                                for (uint32_t it = 0; it < 5; it++) {
                                    uint32_t k = it * 64u + tid;
                                    if (tid < 64 && k < carry) S.tile[k] = cv[it];
                                }
                                __syncthreads();
                                O.tile_base = lim;
                                O.lds_from = lim;
                                O.outpos = carry_end;
                                if (!any_rem) {
                                    O.outpos = w_out1;
                                    break;
                                }
                            } else {
                                O.outpos = w_out1;
                                break;
                            }
                            __syncthreads(); /* X.* is rewritten by the next tile iteration */
                        }
                        __syncthreads();
                    } /* batch */
                    if (status != DEBIG_OK) break;
                    bitpos = wend;
                    if (wflag == FL_EOB) block_done = 1;
                    else if (wflag == FL_TAIL) { block_done = 1; more = 0; }
                    else if (wflag == FL_ERR) { status = wstatus; }
                }
            }
            end_bits = bitpos;
            flush_all(S, O);
            if (status == DEBIG_OK) good = 1;
        }
        if (tid == 0) {
            debig_result r;
            r.final_size = (uint64_t)O.outpos;
            r.good = good;
            r.status = status;
            r.final_set = final_set;
            r.n_blocks = n_blocks;
            r.n_windows = n_windows;
            r.n_rounds = n_rounds;
            r.in_end_bits = (uint64_t)end_bits;
            PROF_STORE(r);
            results[sid] = r;
        }
        __syncthreads();
    }
}
