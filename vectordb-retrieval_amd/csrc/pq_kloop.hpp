// pq_kloop.hpp -- flat PQ<M>, option "pq_kloop": the K-loop scan straight from the product codes for D > 128.
//
// Today a search of a flat PQ index decodes the corpus: pq_panels_kernel (pq.hpp) writes fp16 panels of x^ slab by slab and
// scan16_kloop_kernel (scan16.hpp) reads them back, about 4 N D bytes of traffic per search for an index whose codes are N M bytes.
// This scan reads the codes and gathers its A fragments from the table the panel pass gathers from.  There is no centroid and no slot
// term (the IVF list scan of ivf_pq_kloop.hpp has both): the score is
//     accumulator init                    the resident bias of the panel space (cs ||x^||^2 | 0), as scan16_kloop_kernel
//   + sum_p B[p] T[p]                     T = fp16(sx cb): the handle's pq_tab, copied into the padded form T[m][256][P] with zeros beyond
//                                         dsub; B = fp16(bscale q) in the same padded order (pq_kloop_qpanels_kernel), zero in the padding
// so every product is one the panel pass + scan16_kloop_kernel forms today, the padding adds exact zeros, and bias, sx, maxnorm2,
// corpus_fp16_exact and the bound of DESIGN 4.2 (with Kp accumulation steps in the place of D) serve unchanged: DESIGN 4.9.
//
// Work split, outputs and bins are those of scan16_kloop_kernel: workgroup = 8 waves = one chunk x one 512-query tile in its XCD-aware
// block order ("kloop_qgroup"), a wave owns four 16-query column blocks and, per pass, eight 16-row tiles on
// v_mfma_f32_16x16x32_f16; 8 passes complete the four 256-row bins of a span; the same bin and superbin records, so scan_select, the
// refine tail and the fallback run unchanged.  B fragments stream from L2 per K-step exactly as there.  What is new is how A arrives,
// and that is the list scan's way (ivf_pq_kloop.hpp) on flat rows:
//   codes     a pass is 128 chunk rows x M bytes.  Wave w stages the 16 rows of ITS tile w into LDS one pass ahead of use, the p16 row
//             mapping applied here: MFMA row 4 g + i of tile t of pass (span, slice) is corpus row 1024 span + 256 g + 4 (8 slice + t) + i,
//             so lane group g walks 4 M contiguous bytes of [N][M].  A row at or beyond N reads row 0; its accumulator init is kPadBias.
//             Two passes are resident at pitch CP; a wave reads only what it wrote, so a wave barrier orders it.
//   gather    a tile k-step (16 rows x 32 operand dims of fp16 = 1 KiB) is ONE global_load_lds of 16 bytes per lane with per-lane
//             addresses T + ((m 256 + code) P + 8 sub) 2: the gather from the table IS the staging.  The two code bytes of a lane are
//             read from LDS one K-step before the load is issued, which is BS K-steps before its use.  A piece at or behind Kp reads
//             piece 0 of the table against a zero B operand.  Wave w gathers tile w; all 8 waves consume all 8 tiles with lane-linear
//             ds_read_b128.
// Stage ring and barrier placement: scan16_kloop_kernel's (2 BS stages of 16 KiB, one barrier per BS K-steps); ring depth, code pitch
// and the LDS bytes: pq_kloop_plan.hpp.  NARROW = 1 (batches below 64 queries): MFMAs and select work only for the column blocks
// that hold queries.  Registers, scratch and LDS of the gfx950 compile: profiles/r34_pq_kloop_resources.txt.
#pragma once
#include "pq_kloop_plan.hpp"
#include "scan16.hpp"

namespace vdb {

// pq_tab [M][256][dsub] -> the padded table [M][256][P]: a copy, zero beyond dsub.  Thread per 8-element piece.
__global__ __launch_bounds__(256) void pq_kloop_table_kernel(const _Float16 *__restrict__ tab, int M, int dsub, _Float16 *__restrict__ out) {
    const int P8 = ivf_pqk_p(dsub) / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // piece of entry e = i / P8
    if (i >= (int64_t)M * 256 * P8) return;
    const int64_t e = i / P8;
    const int j0 = (int)(i - e * P8) * 8;
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = j0 + j < dsub ? tab[e * dsub + j0 + j] : (_Float16)0.f;
    *reinterpret_cast<half8 *>(out + i * 8) = o;
}

// B fragments in the padded operand order: build_qpanels16_kernel (prep.hpp) with operand position p = 32 ks + 8 (lane >> 4) + j
// standing for dimension ivf_pqk_operand_dim(p) -- the same product Q bscale, rounded the same way -- and zero where that is none.
// ks32 = 2 nk k-steps per 16-query block.
__global__ __launch_bounds__(256) void pq_kloop_qpanels_kernel(const float *__restrict__ Q, int64_t nq, int D, int M, int dsub, int ks32,
                                                               int64_t nqblocks, const QueryBatchInfo *__restrict__ info,
                                                               half8 *__restrict__ qpanels) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(gid & 63);
    const int64_t tk = gid >> 6;
    const int ks = (int)(tk % ks32);
    const int64_t qb = tk / ks32;
    if (qb >= nqblocks) return;
    const float bs = info->bscale;
    const int64_t q = qb * 16 + (lane & 15);
    const int p0 = ks * 32 + (lane >> 4) * 8;
    half8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = ivf_pqk_operand_dim(p0 + j, M, dsub);
        float v = 0.f;
        if (q < nq && d >= 0) v = Q[(size_t)q * D + d] * bs;
        out[j] = (_Float16)v;
    }
    qpanels[gid] = out;
}

struct PqKloopArgs {
    const unsigned char *codes;   // [N][M], id order
    const _Float16 *table;        // [M][256][P] fp16(sx cb), zero in the padding
    int64_t N;
    int M, P8, npieces;           // P / 8 pieces per table entry; Kp / 8 pieces of a row
};

// a: the flat scan's arguments (`panels` unused, qpanels in the padded order); ex.ksteps = 4 nk.  BS: K-steps between workgroup
// barriers; CP: bytes between staged code rows
template <int BS, int NARROW, int CP>
__global__ __launch_bounds__(512, 2) void pq_kloop_scan_kernel(ScanArgs a, ScanKloopExtra ex, PqKloopArgs pa) {
    constexpr int NWAVES = 8, RING = 2 * BS, HT = 8, CB = 4;
    constexpr int PPS = kTilesPerSpan16 / HT;               // passes per span (8) = passes per 256-row bin
    constexpr int kStageBytes = (int)ivf_pqk_stage_bytes();
    static_assert(HT == NWAVES, "one tile per wave and stage");
    static_assert(BS <= 2, "codes are fetched BS + 1 K-steps ahead, inside the pass after the current one (nk >= 3)");
    static_assert(NARROW == 0 || NARROW == 1, "the LDS-resident query block is not built for this route");
    static_assert((size_t)RING * kStageBytes + (size_t)2 * 128 * CP == pq_kloop_lds_bytes(BS, CP) && pq_kloop_lds_bytes(BS, CP) <= kPqKloopLdsCu,
                  "the plan's LDS bytes");
    __shared__ __attribute__((aligned(16))) unsigned char smem[RING * kStageBytes];
    __shared__ __attribute__((aligned(16))) unsigned char s_codes[2][NWAVES][16][CP];   // [pass & 1][tile][MFMA row][m]

    const int b = blockIdx.x;
    const int x = b & 7, j = b >> 3;
    const int cpx = (a.nchunks + 7) >> 3;                   // chunks per XCD label
    const int per_group = cpx * ex.qgroup;
    const int qg = j / per_group, rem = j - qg * per_group;
    const int ci = rem / ex.qgroup, qt = qg * ex.qgroup + (rem - ci * ex.qgroup);
    if (x + 8 * ci >= a.nchunks || qt >= a.nqtiles) return;
    const int chunk = a.chunk0 + x + 8 * ci;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;                                // lane group = bin of the span
    const int KS = ex.ksteps / 2, nK = KS / 2;              // 32-dim k-steps; 64-dim K-steps of the padded space
    const int64_t q0 = (int64_t)qt * (NWAVES * 16 * CB) + wave * (16 * CB);
    const float cs = a.info->cs;

    const int64_t span0 = chunk_span0(chunk, a.spans_per_chunk, a.chunk_rem);
    int64_t span1 = chunk_span0(chunk + 1, a.spans_per_chunk, a.chunk_rem);
    if (span1 > a.nspans) span1 = a.nspans;
    const int npass = (int)(span1 - span0) * PPS;
    const int nsteps = npass * nK;
    if (nsteps <= 0) return;

    // codes of pass `pass` -> s_codes[pass & 1], this wave's tile: lane group g owns the MFMA rows 4 g + i = four consecutive corpus rows
    const int M = pa.M;
    auto codes_stage = [&](int pass) {
        const int64_t base = (span0 + pass / PPS) * kSpanRows16 + g * kBinRows + 4 * ((pass % PPS) * HT + wave);
        unsigned char *dst = &s_codes[pass & 1][wave][4 * g][0];
        if ((M & 3) == 0) {
            const int mdw = M >> 2;
#pragma unroll 1
            for (int jj = lane & 15; jj < 4 * mdw; jj += 16) {
                const int i = jj / mdw, c = jj - i * mdw;
                const int64_t row = base + i;
                const unsigned char *src = pa.codes + (size_t)(row < pa.N ? row : 0) * M;
                reinterpret_cast<unsigned *>(dst + i * CP)[c] = reinterpret_cast<const unsigned *>(src)[c];
            }
        } else {
#pragma unroll 1
            for (int jj = lane & 15; jj < 4 * M; jj += 16) {
                const int i = jj / M, c = jj - i * M;
                const int64_t row = base + i;
                dst[i * CP + c] = pa.codes[(size_t)(row < pa.N ? row : 0) * M + c];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // (a wave reads only the rows it staged itself)
        __builtin_amdgcn_wave_barrier();
    };

    // The two pieces of this lane in K-step `step`: lane (r, kq) of k-step ks -> piece pc = 8 kk + 4 ks + kq, of sub-space m = pc / P8.
    // code_fetch reads their code bytes (one register); stage_issue forms the table addresses and gathers this wave's tile of the
    // K-step into LDS slot `buf`: the piece of lane (r, kq) lands at byte 16 lane of (tile, ks)
    const float inv_p8 = 1.0f / (float)pa.P8;
    auto piece_m = [&](int pc) { return (int)(((float)pc + 0.5f) * inv_p8); };   // pc / P8: pc < 512, the quotient is 0.5 / P8 away from an integer
    auto code_fetch = [&](int step) {
        const int pass = step / nK, kk = step - pass * nK;
        const unsigned char *cr = &s_codes[pass & 1][wave][lane & 15][0];
        const int pc = 8 * kk + g;
        const unsigned c0 = cr[pc < pa.npieces ? piece_m(pc) : 0], c1 = cr[pc + 4 < pa.npieces ? piece_m(pc + 4) : 0];
        return c0 | (c1 << 8);
    };
    const unsigned char *tab = reinterpret_cast<const unsigned char *>(pa.table);
    auto stage_issue = [&](int step, unsigned cpair, int buf) {
        const int kk = step % nK;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int pc = 8 * kk + 4 * ks + g, m = piece_m(pc);
            const int code = (int)((cpair >> (8 * ks)) & 255u);
            const int off = pc < pa.npieces ? ((m * 256 + code) * pa.P8 + (pc - m * pa.P8)) * 16 : 0;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1))) void *>(reinterpret_cast<uintptr_t>(tab + off)),
                reinterpret_cast<__attribute__((address_space(3))) void *>(
                    static_cast<uint32_t>(reinterpret_cast<uintptr_t>(smem + buf * kStageBytes + (wave * 2 + ks) * 1024))),
                16, 0, 0);
        }
    };
    auto clamp_step = [&](int s) { return s < nsteps ? s : nsteps - 1; };

    codes_stage(0);
#pragma unroll
    for (int i = 0; i < BS; ++i)
        if (i < nsteps) stage_issue(i, code_fetch(i), i);
    unsigned pre = code_fetch(clamp_step(BS));
    // A wave whose 64 query columns are all padding keeps its tile's codes, gathers and the barriers going and nothing else
    // (scan16_kloop_kernel: a single query costs one wave's matrix work per workgroup)
    if (a.nq_valid > 0 && q0 >= a.nq_valid) {
        __syncthreads();
        for (int step = 0; step < nsteps; ++step) {
            const int pass = step / nK;
            if (step == pass * nK && pass + 1 < npass) codes_stage(pass + 1);
            stage_issue(clamp_step(step + BS), pre, (step + BS) % RING);
            pre = code_fetch(clamp_step(step + 1 + BS));
            if (BS == 1 || (step % BS) == BS - 1) __syncthreads();
        }
        return;
    }

    const float INF = __builtin_inff();
    float NEG_INF = -INF;
    asm volatile("" : "+v"(NEG_INF));
    unsigned idmask = kQuadIdMask;
    asm volatile("" : "+v"(idmask));
    float m1[CB], m2[CB], M1[CB], M2[CB];
    int Ms[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        m1[cb] = m2[cb] = M1[cb] = M2[cb] = INF;
        Ms[cb] = 0;
    }

    float4v acc[HT][CB];
    half8 bq[CB][2];          // B fragments of the current K-step, reloaded in place (scan16.hpp)
    const int lane16 = lane * 16;
    const __amdgpu_buffer_rsrc_t rsq = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<half8 *>(a.qpanels + (size_t)(q0 / 16) * KS * 64), 0, 0x7fffffff, 0x00020000);
    auto load_b = [&](int kk, int ks) {
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
            bq[cb][ks] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsq, lane16, (cb * KS + kk * 2 + ks) * 1024, 0));
    };
    // column blocks of this wave that hold queries (wave-uniform)
    const int ncb = !NARROW ? CB : __builtin_amdgcn_readfirstlane((int)((a.nq_valid - q0 + 15) / 16 < CB ? (a.nq_valid - q0 + 15) / 16 : CB));
    load_b(0, 0);
    __syncthreads();

    half8 fr[2][4];
    auto read_group = [&](int buf, int grp, half8(&dst)[4]) {   // group grp = (ks = grp >> 1, tiles 4 (grp & 1) .. + 3)
        const half8 *A = reinterpret_cast<const half8 *>(smem + buf * kStageBytes);
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t] = A[(((grp & 1) * 4 + t) * 2 + (grp >> 1)) * 64 + lane];
    };
    read_group(0, 0, fr[0]);

    int step = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int64_t span = span0 + pass / PPS;
        const int slice = pass % PPS;
        if (pass + 1 < npass) codes_stage(pass + 1);
        // accumulators start from the bias of their rows: row = 1024 span + 256 g + 4 (HT slice + t) + i
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const float4 c = *reinterpret_cast<const float4 *>(a.bias + span * kSpanRows16 + g * kBinRows + (slice * HT + t) * 4);
            acc[t][0][0] = (c.x >= 0.9e38f) ? kPadBias : c.x * cs;
            acc[t][0][1] = (c.y >= 0.9e38f) ? kPadBias : c.y * cs;
            acc[t][0][2] = (c.z >= 0.9e38f) ? kPadBias : c.z * cs;
            acc[t][0][3] = (c.w >= 0.9e38f) ? kPadBias : c.w * cs;
#pragma unroll
            for (int cb = 1; cb < CB; ++cb) acc[t][cb] = acc[t][0];
        }
#pragma unroll 1
        for (int kk = 0; kk < nK; ++kk, ++step) {
            const int buf = step % RING;
            load_b(kk, 1);
            stage_issue(clamp_step(step + BS), pre, (step + BS) % RING);
            const int kn = (kk + 1 == nK) ? 0 : kk + 1;      // B repeats every pass
#pragma unroll
            for (int grp = 0; grp < 4; ++grp) {
                __builtin_amdgcn_sched_barrier(0);
                if (grp < 3) {
                    read_group(buf, grp + 1, fr[(grp + 1) & 1]);
                    if (grp == 1) pre = code_fetch(clamp_step(step + 1 + BS));   // (the codes of the gather after next: off the MFMA path)
                } else {
                    if (BS == 1 || (step % BS) == BS - 1) __syncthreads();
                    read_group((step + 1) % RING, 0, fr[0]);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (!NARROW) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int cb = 0; cb < CB; ++cb)
                            acc[(grp & 1) * 4 + t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                fr[grp & 1][t], bq[cb][grp >> 1], acc[(grp & 1) * 4 + t][cb], 0, 0, 0);
                } else {
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
                        if (cb < ncb) {
#pragma unroll
                            for (int t = 0; t < 4; ++t)
                                acc[(grp & 1) * 4 + t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                    fr[grp & 1][t], bq[cb][grp >> 1], acc[(grp & 1) * 4 + t][cb], 0, 0, 0);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (grp == 1) load_b(kn, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < HT; ++t) {
            const unsigned id = (unsigned)(slice * HT + t);  // quad number inside the 256-row bin
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                if (NARROW && cb >= ncb) continue;           // (its minima stay +inf: nothing reads those columns)
                const float qm = quad_min(acc[t][cb][0], acc[t][cb][1], acc[t][cb][2], acc[t][cb][3], NEG_INF);
                const float v = pack_score(qm, idmask, id);
                m2[cb] = __builtin_amdgcn_fmed3f(m1[cb], m2[cb], v);
                m1[cb] = fast_min(m1[cb], v, NEG_INF);
            }
        }
        if (slice == PPS - 1) {                              // the four bins (span, g) are complete
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const size_t o = (size_t)(span * 4 + g) * a.Qpad + q0 + cb * 16 + (lane & 15);
                a.bin_m1[o] = m1[cb];
                a.bin_m2[o] = m2[cb];
                M2[cb] = __builtin_fminf(__builtin_amdgcn_fmed3f(M1[cb], M2[cb], m1[cb]), m2[cb]);
                if (m1[cb] < M1[cb]) Ms[cb] = (int)span;
                M1[cb] = __builtin_fminf(M1[cb], m1[cb]);
                m1[cb] = INF;
                m2[cb] = INF;
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const size_t so = (size_t)(chunk * 4 + g) * a.Qpad + q0 + cb * 16 + (lane & 15);
        a.sb_m1[so] = M1[cb];
        a.sb_m2[so] = M2[cb];
        a.sb_span[so] = Ms[cb];
    }
}

}  // namespace vdb
