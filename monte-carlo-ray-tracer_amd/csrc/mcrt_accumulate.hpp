// Accumulated rendering (include/mcrt.h mcrt_frame_merge*): the text of the one gfx950 kernel of mcrt_accumulate.hip, shared with the
// host emulation of the CPU tests (tests/emu/accumulate_emu.cpp): both run this file. Only FP64 + - * /, compare and select, in the order
// include/mcrt.h states, built uncontracted like the rest of the exact build.
//
// frameMergeKernel is a lane per pixel: the summaries of two sample sets of the pixel in, the summary of their concatenation out. The
// three channel groups are worked through one after the other - load, compute, store - so nothing lives from one group into the next
// and the register peak is the highlights group's alone: the list as four (luminance, rgb) places in named registers, every entry of B
// one unrolled compare-select insertion, no array that a run-time index could send to scratch. Which groups are present is uniform
// over the launch: plain branches on the pointers. A lane's 24 B of a frame are 8-byte aligned only (odd pixels start at 8 mod 16), so
// a record is three 8-byte loads per lane, as in robustHighlightsKernel; a wave reads 1 536 consecutive bytes of a frame either way. A
// lane reads everything of a group before it writes, and only its own pixel: every output may be the same buffer of A.
#pragma once

#include "../../include/mcrt.h"
#include "mcrt_math.hpp"
#include "mcrt_robust.hpp"

namespace mcrt {

constexpr uint32_t kFrameMergeBlock = 256;  // lanes of a workgroup; each owns a pixel
constexpr uint32_t kFrameMergeTopsMin = 4 * MCRT_ROBUST_TOPS;  // samples per side from which its list is full
static_assert(MCRT_ROBUST_TOPS == 4, "the list is four named places");

// One merge: `pixels` pixels of A (n_a samples each) followed by B (n_b samples each). A group is worked on when its output is set.
struct FrameMerge {
    mcrt_frame_summary a, b, out;  // out.x may be a.x
    uint64_t pixels;
    uint32_t n_a, n_b;
};

// include/mcrt.h's wmean: a term whose count is 0 takes no part (a select on the launch-uniform counts).
MCRT_HD double mergeWeighted(uint32_t c1, double x1, uint32_t c2, double x2) {
    const double w1 = (double)c1 * x1, w2 = (double)c2 * x2;
    return (c1 > 0 ? (c2 > 0 ? w1 + w2 : w1) : w2) / (double)(c1 + c2);
}

// A place of the list: luminance and rgb.
struct MergeEntry {
    double l, r, g, b;
};
MCRT_HD MergeEntry mergeEntry(const double* p) { return MergeEntry{robustLuminance(p[0], p[1], p[2]), p[0], p[1], p[2]}; }
MCRT_HD MergeEntry mergePick(bool c, const MergeEntry& x, const MergeEntry& y) {
    return MergeEntry{c ? x.l : y.l, c ? x.r : y.r, c ? x.g : y.g, c ? x.b : y.b};
}
// Entry x goes before the first place it exceeds (b_j: "at or before place j" - true from the insertion place on, the list being
// sorted); the place pushed past 3 leaves, or x itself when it exceeds none. Returns the luminance of what left.
MCRT_HD double mergeInsert(MergeEntry& e0, MergeEntry& e1, MergeEntry& e2, MergeEntry& e3, const MergeEntry& x) {
    const bool b0 = x.l > e0.l, b1 = b0 || x.l > e1.l, b2 = b1 || x.l > e2.l, b3 = b2 || x.l > e3.l;
    const double gone = b3 ? e3.l : x.l;
    e3 = mergePick(b2, e2, mergePick(b3, x, e3));
    e2 = mergePick(b1, e1, mergePick(b2, x, e2));
    e1 = mergePick(b0, e0, mergePick(b1, x, e1));
    e0 = mergePick(b0, x, e0);
    return gone;
}

MCRT_HD void frameMergeLane(const FrameMerge& fm, uint64_t pixel) {
    if (pixel >= fm.pixels) return;
    const uint32_t n_a = fm.n_a, n_b = fm.n_b;
    const double a = (double)n_a, b = (double)n_b, t = a + b;
    if (fm.out.rgb) {
        const double* pa = fm.a.rgb + pixel * 3;
        const double* pb = fm.b.rgb + pixel * 3;
        const double ma_r = pa[0], ma_g = pa[1], ma_b = pa[2];
        const double mb_r = pb[0], mb_g = pb[1], mb_b = pb[2];
        if (fm.out.variance) {
            const double* va = fm.a.variance + pixel * 3;
            const double* vb = fm.b.variance + pixel * 3;
            const double va_r = va[0], va_g = va[1], va_b = va[2];
            const double vb_r = vb[0], vb_g = vb[1], vb_b = vb[2];
            const double d_r = mb_r - ma_r, d_g = mb_g - ma_g, d_b = mb_b - ma_b;
            const double w = (a * b) / t;
            double* o = fm.out.variance + pixel * 3;
            o[0] = (((a - 1.0) * va_r + (b - 1.0) * vb_r) + (d_r * d_r) * w) / (t - 1.0);
            o[1] = (((a - 1.0) * va_g + (b - 1.0) * vb_g) + (d_g * d_g) * w) / (t - 1.0);
            o[2] = (((a - 1.0) * va_b + (b - 1.0) * vb_b) + (d_b * d_b) * w) / (t - 1.0);
        }
        double* o = fm.out.rgb + pixel * 3;
        o[0] = (a * ma_r + b * mb_r) / t;
        o[1] = (a * ma_g + b * mb_g) / t;
        o[2] = (a * ma_b + b * mb_b) / t;
    }
    if (fm.out.half_a) {
        const uint32_t e_a = (n_a + 1) / 2, o_a = n_a / 2, e_b = (n_b + 1) / 2, o_b = n_b / 2;
        const bool swap = (n_a & 1u) != 0;  // B's even samples become odd ones
        const double* pe = (swap ? fm.b.half_b : fm.b.half_a) + pixel * 3;  // what of B joins the even samples
        const double* po = (swap ? fm.b.half_a : fm.b.half_b) + pixel * 3;
        const uint32_t c_e = swap ? o_b : e_b, c_o = swap ? e_b : o_b;
        const double* ha = fm.a.half_a + pixel * 3;
        const double* hb = fm.a.half_b + pixel * 3;
        const double ha_r = ha[0], ha_g = ha[1], ha_b = ha[2], hb_r = hb[0], hb_g = hb[1], hb_b = hb[2];
        const double pe_r = pe[0], pe_g = pe[1], pe_b = pe[2], po_r = po[0], po_g = po[1], po_b = po[2];
        double* oa = fm.out.half_a + pixel * 3;
        double* ob = fm.out.half_b + pixel * 3;
        oa[0] = mergeWeighted(e_a, ha_r, c_e, pe_r);
        oa[1] = mergeWeighted(e_a, ha_g, c_e, pe_g);
        oa[2] = mergeWeighted(e_a, ha_b, c_e, pe_b);
        ob[0] = mergeWeighted(o_a, hb_r, c_o, po_r);
        ob[1] = mergeWeighted(o_a, hb_g, c_o, po_g);
        ob[2] = mergeWeighted(o_a, hb_b, c_o, po_b);
    }
    if (fm.out.tops) {
        const double* ta = fm.a.tops + pixel * (MCRT_ROBUST_TOPS * 3);
        const double* tb = fm.b.tops + pixel * (MCRT_ROBUST_TOPS * 3);
        MergeEntry e0 = mergeEntry(ta), e1 = mergeEntry(ta + 3), e2 = mergeEntry(ta + 6), e3 = mergeEntry(ta + 9);
        const MergeEntry x0 = mergeEntry(tb), x1 = mergeEntry(tb + 3), x2 = mergeEntry(tb + 6), x3 = mergeEntry(tb + 9);
        const double level_a = fm.a.level[pixel], level_b = fm.b.level[pixel];
        double gone = 0.0;
        gone = gone + mergeInsert(e0, e1, e2, e3, x0);
        gone = gone + mergeInsert(e0, e1, e2, e3, x1);
        gone = gone + mergeInsert(e0, e1, e2, e3, x2);
        gone = gone + mergeInsert(e0, e1, e2, e3, x3);
        double* o = fm.out.tops + pixel * (MCRT_ROBUST_TOPS * 3);
        o[0] = e0.r, o[1] = e0.g, o[2] = e0.b;
        o[3] = e1.r, o[4] = e1.g, o[5] = e1.b;
        o[6] = e2.r, o[7] = e2.g, o[8] = e2.b;
        o[9] = e3.r, o[10] = e3.g, o[11] = e3.b;
        fm.out.level[pixel] = (((a - 4.0) * level_a + (b - 4.0) * level_b) + gone) / (t - 4.0);
    }
}

// What mcrt_frame_merge* refuses about the channels and the counts, for the library and the emulation alike: MCRT_OK, or the status
// with *why set.
inline int frameMergeCheck(uint64_t pixels, const mcrt_frame_summary* a, uint32_t n_a, const mcrt_frame_summary* b, uint32_t n_b,
                           const mcrt_frame_summary* out, const char** why) {
    const char* sink;
    if (!why) why = &sink;
    if (!a || !b || !out) return *why = "a summary is NULL", MCRT_ERR_INVALID;
    if (pixels == 0 || pixels > 0xFFFFFFFFull) return *why = "pixels must be non-zero and below 2^32", MCRT_ERR_INVALID;
    if (n_a == 0 || n_b == 0) return *why = "a sample count is 0", MCRT_ERR_INVALID;
    if ((uint64_t)n_a + n_b > 0xFFFFFFFFull) return *why = "n_a + n_b does not fit uint32_t", MCRT_ERR_INVALID;
    if (out->variance && !out->rgb) return *why = "the variance needs rgb", MCRT_ERR_INVALID;
    if (!out->half_a != !out->half_b) return *why = "half_a and half_b are wanted together", MCRT_ERR_INVALID;
    if (!out->tops != !out->level) return *why = "tops and level are wanted together", MCRT_ERR_INVALID;
    if (!out->rgb && !out->half_a && !out->tops) return *why = "no channel group is wanted", MCRT_ERR_INVALID;
    if (out->rgb && (!a->rgb || !b->rgb)) return *why = "rgb is wanted and an input's is NULL", MCRT_ERR_INVALID;
    if (out->variance && (!a->variance || !b->variance)) return *why = "variance is wanted and an input's is NULL", MCRT_ERR_INVALID;
    if (out->half_a && (!a->half_a || !a->half_b || !b->half_a || !b->half_b)) return *why = "the halves are wanted and an input's are NULL", MCRT_ERR_INVALID;
    if (out->tops && (!a->tops || !a->level || !b->tops || !b->level)) return *why = "the highlights are wanted and an input's are NULL", MCRT_ERR_INVALID;
    if (out->tops && (n_a < kFrameMergeTopsMin || n_b < kFrameMergeTopsMin))
        return *why = "the highlights need 16 samples on both sides", MCRT_ERR_UNSUPPORTED;
    return MCRT_OK;
}

}  // namespace mcrt
