// niti_grouped_host.hip -- the one host front of the grouped 3x3 conv layers (gconv_*, niti_kernels.hpp): the shape
// predicate, the slab-count plan of the weight gradient and the two launches, written once over the record each
// kernel family exports (GcKernels, niti_grouped.hpp).  The group width picks the family (gc_width); what a family
// does with a launch is in its own file: niti_grouped.hip, niti_grouped_narrow.hip, niti_grouped_packed.hip.
#include <algorithm>

#include "niti_grouped.hpp"
#include "niti_kernels.hpp"

namespace niti {

namespace {

const GcKernels& gc_kernels(GcFamily f) { return f == GC_NARROW ? gc_narrow() : f == GC_PACKED ? gc_packed() : gc_wide(); }

inline int gc_bands(int rows) { return (rows + 3) / 4; }

// what every family asks of (g, groups) but the group width and the slab bound; the two maps below 2^31 bytes
bool gconv_shape_ok(const ConvGeom& g, int groups, bool pitch16) {
    if (groups < 2 || groups > 65535 || g.n < 1 || g.c_in < 1 || g.c_in != g.c_out || g.c_in % groups != 0) return false;
    if (g.kh != 3 || g.kw != 3 || g.sh < 1 || g.sh > 2 || g.sw != g.sh || g.dh != 1 || g.dw != 1) return false;
    if (g.pt < 0 || g.pt > 2 || g.pl != g.pt || g.pb != g.pt || g.pr != g.pt) return false;
    if (g.h < 1 || g.w < 1 || g.h + 2 * g.pt < 3 || g.w + 2 * g.pt < 3) return false;
    if (g.oh != (g.h + 2 * g.pt - 3) / g.sh + 1 || g.ow != (g.w + 2 * g.pt - 3) / g.sh + 1) return false;
    if (g.cip != (pitch16 ? (g.c_in + 15) / 16 * 16 : g.c_in) || g.cop != g.cip) return false;
    const int64_t lim = (int64_t)1 << 31;
    return (int64_t)g.n * g.h * g.w * g.cip < lim && (int64_t)g.n * g.oh * g.ow * g.cop < lim;
}

// the slabs of the weight gradient, a function of the shape alone: one per unit (image, band, segment) up to a cap
// of GC_SLAB_BYTES of slabs, 64 at the least, GC_MAX_SLABS at the most, and what the family's grid asks on top
int gc_plan(const ConvGeom& g, int groups) {
    const int cg = g.c_in / groups;
    const GcWidth wd = gc_width(cg);
    const GcKernels& f = gc_kernels(wd.family);
    const int64_t units = (int64_t)g.n * gc_bands(g.oh) * f.segs(g.ow, cg, g.sh);
    const int64_t one = (int64_t)g.c_out * 9 * wd.cgp * sizeof(int32_t);
    const int64_t cap = std::max<int64_t>({64, std::min<int64_t>(GC_MAX_SLABS, (int64_t)GC_SLAB_BYTES / one),
                                           f.min_workgroups / f.grid_y(g.c_in, groups)});
    return (int)std::max<int64_t>(1, std::min<int64_t>(cap, units));
}

bool gc_ok(const ConvGeom& g, int groups, GcFamily only) {
    return gconv_any_ok(g, groups) && gc_width(g.c_in / groups).family == only;
}

hipError_t gc_act(const ConvGeom& g, int groups, bool dgrad, const int8_t* in, const int8_t* w, uint32_t* amax,
                  const ActOut& o, int pass, hipStream_t st) {
    if (!gconv_any_ok(g, groups) || in == nullptr || w == nullptr || amax == nullptr || pass < 0 || pass > 1)
        return hipErrorInvalidValue;
    // the fields this launch honours: out, relu (forward), relu_mask (input gradient), the exponents
    if (o.pool.pool_out != nullptr || o.pool.x != nullptr || o.pool.y != nullptr || o.pool.dx != nullptr ||
        o.pool.dx_c32 != nullptr || o.out_p16 != nullptr || o.zero_cls != 0 || o.pool3.out != nullptr ||
        o.pool3.arg != nullptr)
        return hipErrorInvalidValue;
    if ((dgrad && o.relu != 0) || (!dgrad && o.relu_mask != nullptr)) return hipErrorInvalidValue;
    if (pass == 1 && o.out == nullptr) return hipErrorInvalidValue;
    const int cg = g.c_in / groups;
    const GcWidth wd = gc_width(cg);
    const GcKernels& f = gc_kernels(wd.family);
    const bool d2 = dgrad && g.sh == 2;
    GcActArgs a{};
    a.x = in;
    a.w = w;
    a.out = o.out;
    a.relu_mask = o.relu_mask;
    a.C = g.c_in;
    a.cp = wd.pitch16 ? g.cip : 0;
    a.ih = dgrad ? g.oh : g.h;
    a.iw = dgrad ? g.ow : g.w;
    a.oh = dgrad ? g.h : g.oh;
    a.ow = dgrad ? g.w : g.ow;
    // the input gradient at stride 1: the same conv on dy, taps reversed; at stride 2: the layer's own pad
    a.pad = dgrad && !d2 ? 2 - g.pt : g.pt;
    a.relu = o.relu;
    a.xbytes = (uint32_t)((int64_t)g.n * a.ih * a.iw * g.cip);
    a.wbytes = (uint32_t)((int64_t)g.c_out * 9 * wd.cgp);
    // bands / segments over the output; the stride-2 input gradient: over ((y + pad) / 2, (x + pad) / 2)
    a.bands = gc_bands(d2 ? (g.h - 1 + g.pt) / 2 + 1 : a.oh);
    a.segs = f.segs(d2 ? (g.w - 1 + g.pt) / 2 + 1 : a.ow, cg, g.sh);
    a.amax = amax;
    a.exp_in = o.exp_in;
    a.wscale = o.wscale;
    a.exp_out = o.exp_out;
    const int64_t gx = (int64_t)g.n * a.bands * a.segs;
    if (gx > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f.act(cg, g.sh, dgrad, pass), dim3((unsigned)gx, f.grid_y(g.c_in, groups)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

bool gconv_any_ok(const ConvGeom& g, int groups) {
    const GcWidth wd = gc_width(groups > 0 ? g.c_in / groups : 0);
    if (wd.family == GC_NONE || !gconv_shape_ok(g, groups, wd.pitch16)) return false;
    // (the two maps: gconv_shape_ok) the slab buffer the weight gradient writes, below 2^31 bytes
    return (int64_t)gc_plan(g, groups) * g.c_out * 9 * wd.cgp * 4 < ((int64_t)1 << 31);
}

bool gconv_ok(const ConvGeom& g, int groups) { return g.sh == 1 && g.sw == 1 && gc_ok(g, groups, GC_WIDE); }
bool gconv2_ok(const ConvGeom& g, int groups) { return gc_ok(g, groups, GC_WIDE); }
bool gconv_narrow_ok(const ConvGeom& g, int groups) { return gc_ok(g, groups, GC_NARROW); }
bool gconv_packed_ok(const ConvGeom& g, int groups) { return gc_ok(g, groups, GC_PACKED); }

hipError_t gconv_fwd(const ConvGeom& g, int groups, const int8_t* x, const int8_t* w, uint32_t* amax, const ActOut& o,
                     int pass, hipStream_t st) {
    return gc_act(g, groups, false, x, w, amax, o, pass, st);
}

hipError_t gconv_dgrad(const ConvGeom& g, int groups, const int8_t* dy, const int8_t* w, uint32_t* amax,
                       const ActOut& o, int pass, hipStream_t st) {
    return gc_act(g, groups, true, dy, w, amax, o, pass, st);
}

int gconv_wgrad_slabs(const ConvGeom& g, int groups) { return gconv_any_ok(g, groups) ? gc_plan(g, groups) : 0; }

hipError_t gconv_wgrad(const ConvGeom& g, int groups, const int8_t* x, const int8_t* dy, int32_t* slab,
                       size_t slab_bytes, int* slabs, hipStream_t st, SgdJob* defer) {
    if (!gconv_any_ok(g, groups) || x == nullptr || dy == nullptr || slab == nullptr) return hipErrorInvalidValue;
    const int cg = g.c_in / groups;
    const GcWidth wd = gc_width(cg);
    const GcKernels& f = gc_kernels(wd.family);
    const int ns = gc_plan(g, groups);
    const size_t one = (size_t)g.c_out * 9 * wd.cgp;  // elements of a slab
    if (ns * one * sizeof(int32_t) > slab_bytes) return hipErrorInvalidValue;
    GcWgArgs a{};
    a.x = x;
    a.dy = dy;
    a.slab = slab;
    a.xbytes = (uint32_t)((int64_t)g.n * g.h * g.w * g.cip);
    a.dbytes = (uint32_t)((int64_t)g.n * g.oh * g.ow * g.cop);
    a.h = g.h;
    a.w = g.w;
    a.oh = g.oh;
    a.ow = g.ow;
    a.C = g.c_in;
    a.cp = wd.pitch16 ? g.cip : 0;
    a.pad = g.pt;
    a.bands = gc_bands(g.oh);
    a.segs = f.segs(g.ow, cg, g.sh);
    a.units = g.n * a.bands * a.segs;
    hipLaunchKernelGGL(f.wgrad(cg, g.sh), dim3((unsigned)ns, f.grid_y(g.c_in, groups), f.wgrad_z(cg)), dim3(256), 0, st, a);
    if (slabs != nullptr) *slabs = ns;
    if (defer != nullptr) {  // C-shaped slabs for the update launch's combine
        defer->slab = slab;
        defer->splits = ns;
        defer->slab_stride = (int64_t)one;
        defer->slab_n = (int64_t)one;
        defer->slab_map = 0;
    }
    return hipGetLastError();
}

}  // namespace niti
