// vr_variant.h — which kernel a launch runs, stated once.
//
// A frame (or a vr_count_work pass) runs one instantiation of march_kernel, march_pair_kernel,
// mip_kernel, iso_kernel, proj_kernel or march_y_kernel: a FrameVariant.  resolve_variant is the only place the mapping from
// a launch's resolved inputs (VariantFacts) to it is written, variant_built the only list of the
// instantiations the library carries; the launch (launch_frame, vr_kernels.hip), the name a
// profiler reports and the tile-schedule key all derive from the one FrameVariant.  The policy
// -- which facts a view gets -- is not here (use_pipeline, use_grad_field, use_pair, want_alt,
// mip_inflight, iso_inflight, proj_inflight in vr_api.hip).  Plain C++17, no HIP types.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/vr/vr_debug.h"
#include "../../include/vr/vr_modes.h"

namespace vr {

// Layout codes (the layouts themselves: vr_internal.h).  A base layout is a storage type, or
// an 8-bit one | kQuadFlag; an alternative f32 copy is ST_F32 | one of the four copy flags.
enum StorageType { ST_U8 = 0, ST_I8 = 1, ST_U16 = 2, ST_I16 = 3, ST_F32 = 4 };
constexpr int kQuadFlag = 0x10, kAltFlag = 0x20, kPlainF32Flag = 0x100, kStencilF32Flag = 0x200,
              kYMajorFlag = 0x400;
constexpr int kTfLds = 256;  // TF texels staged in LDS (lane groups and pipelining need it there)

enum VariantFamily { VF_NONE = -1, VF_MARCH = 0, VF_PAIR = 1, VF_MIP = 2, VF_ISO = 3, VF_MARCH_Y = 4,
                     VF_PROJ = 5 };
constexpr int kVariantFamilies = 6;
// The kernels' storage type tag (their first template argument): kTagNames and launch_frame's
// type list follow this order.  TAG_F32H: the ST_F32 bricks read with the binary16 field.
// TAG_F32Y / TAG_F32HY: the y-major copy (kYMajorFlag), unshaded / shaded with the binary16
// field; march_y_kernel's only tags, and no other family takes them.
enum VariantTag {
    TAG_U8, TAG_I8, TAG_U16, TAG_I16, TAG_F32, TAG_QUAD_U8, TAG_QUAD_I8,
    TAG_F32ALT, TAG_F32H, TAG_F32P, TAG_F32S, TAG_F32Y, TAG_F32HY, kVariantTags
};
constexpr const char *kTagNames[kVariantTags] = {
    "unsigned char", "signed char", "unsigned short", "short", "float",
    "vr::Quad8<unsigned char>", "vr::Quad8<signed char>", "vr::F32Alt", "vr::F32H", "vr::F32P",
    "vr::F32S", "vr::F32Y", "vr::F32HY"};

// march_kernel<VT, shade, count, skip, gf, pipe>, march_pair_kernel<VT, shade, gf, lanes>,
// mip_kernel<VT, count, skip, inflight>, iso_kernel<VT, count, skip, inflight>,
// proj_kernel<VT, op, count, skip, inflight> or march_y_kernel<VT, shade> (the pipelined
// single-lane march, gf = shade); what a family does not take stays false / 0.
struct FrameVariant {
    int family = VF_NONE, tag = 0;
    bool shade = false, count = false, skip = false, gf = false, pipe = false;
    int lanes = 0;     // lanes per ray: 2 or 4
    int inflight = 0;  // samples of a ray in flight: 1, 2 or 4
    int op = 0;        // proj_kernel: kProjMin or kProjMean
};
constexpr int kProjMin = 0, kProjMean = 1;  // proj_kernel's OP (VR_MODE_MINIP, VR_MODE_MEAN)
// proj_strip's third operator, the maximum: mip_kernel's strip only, never a FrameVariant::op
// (VF_MIP stays a family of its own and no proj_kernel<VT, kProjMax, ...> is built)
constexpr int kProjMax = 2;

// The resolved inputs of the decision, after the derived structures a launch reads were built
// or refused (the fields: vr_debug.h).
using VariantFacts = ::vr_variant_facts;

// false (*v stays VF_NONE): no kernel serves these facts, the launch is hipErrorInvalidValue.
inline bool resolve_variant(const VariantFacts &f, FrameVariant *v)
{
    *v = FrameVariant{};
    const int base = f.layout >= ST_U8 && f.layout <= ST_F32 ? f.layout
                     : f.layout == (ST_U8 | kQuadFlag)       ? TAG_QUAD_U8
                     : f.layout == (ST_I8 | kQuadFlag)       ? TAG_QUAD_I8
                                                             : -1;
    const int alt = f.layout == (ST_F32 | kAltFlag)          ? TAG_F32ALT
                    : f.layout == (ST_F32 | kPlainF32Flag)   ? TAG_F32P
                    : f.layout == (ST_F32 | kStencilF32Flag) ? TAG_F32S
                                                             : -1;
    if (f.layout == (ST_F32 | kYMajorFlag)) {
        // the y-major copy: composite frames, pipelined, one lane per ray, TF in LDS; shaded
        // ones read the shared binary16 field, unshaded ones none
        if (f.mode != VR_MODE_COMPOSITE || f.count || f.pair || f.skip || !f.pipeline ||
            f.tf_n > kTfLds || (f.shade ? !(f.field && f.field_half) : f.field != 0))
            return false;
        *v = {VF_MARCH_Y, f.shade ? (int)TAG_F32HY : (int)TAG_F32Y, f.shade != 0, false, false,
              f.shade != 0, true, 0, 0};
        return true;
    }
    if (f.mode == VR_MODE_MIP || f.mode == VR_MODE_ISO) {  // base layouts only: no alternative copy
        const int k = f.count ? 1 : f.mip_inflight;  // the counting kernels walk step by step
        if (base < 0 || (k != 1 && k != 2 && k != 4)) return false;
        *v = {f.mode == VR_MODE_ISO ? VF_ISO : VF_MIP, base, false, f.count != 0, f.skip != 0, false,
              false, 0, k};
        return true;
    }
    if (f.mode == VR_MODE_MINIP || f.mode == VR_MODE_MEAN) {  // base layouts only, as MIP
        const int k = f.count ? 1 : f.mip_inflight;
        if (base < 0 || (k != 1 && k != 2 && k != 4)) return false;
        *v = {VF_PROJ, base, false, f.count != 0, f.skip != 0, false, false, 0, k,
              f.mode == VR_MODE_MEAN ? kProjMean : kProjMin};
        return true;
    }
    // an alternative copy carries no skip-empty structures, field or lane groups, and no counts
    if (base < 0 && (alt < 0 || f.count || f.pair || f.skip || f.field)) return false;
    const bool gf = base == TAG_F32 && f.shade && f.field;  // shaded f32 launches read the field
    const int tag = alt >= 0 ? alt : gf && f.field_half ? (int)TAG_F32H : base;
    if (f.pair)  // (the policy grants lane groups to frames without skip-empty, TF in LDS)
        *v = {VF_PAIR, tag, f.shade != 0, false, false, gf, false, f.pair == 4 ? 4 : 2, 0};
    else
        *v = {VF_MARCH, tag, f.shade != 0, f.count != 0, f.skip != 0, gf,
              f.pipeline && !f.count && !f.skip && f.tf_n <= kTfLds, 0, 0};
    return true;
}

// The instantiations the library carries: 92 march_kernel, 32 march_pair_kernel, 56 mip_kernel,
// 56 iso_kernel, 2 march_y_kernel, 112 proj_kernel.
constexpr bool variant_built(const FrameVariant &v)
{
    const bool alt = v.tag == TAG_F32ALT || v.tag == TAG_F32P || v.tag == TAG_F32S;
    const bool field_type = v.tag == TAG_F32 || v.tag == TAG_F32H;
    if (v.tag < 0 || v.tag >= kVariantTags) return false;
    if (v.family == VF_MARCH_Y)
        return v.tag == (v.shade ? TAG_F32HY : TAG_F32Y) && v.gf == v.shade && v.pipe && !v.count &&
               !v.skip;
    if (v.tag == TAG_F32Y || v.tag == TAG_F32HY) return false;
    if (v.gf ? !(v.shade && field_type) : v.tag == TAG_F32H) return false;  // F32H: gf only
    switch (v.family) {
        case VF_MARCH: return !(v.pipe && (v.count || v.skip)) && !(alt && (v.count || v.skip));
        case VF_PAIR: return !alt && (v.lanes == 2 || v.lanes == 4);
        case VF_MIP:
        case VF_ISO: return !alt && (v.inflight == 1 || (!v.count && (v.inflight == 2 || v.inflight == 4)));
        case VF_PROJ:
            return !alt && (v.op == kProjMin || v.op == kProjMean) &&
                   (v.inflight == 1 || (!v.count && (v.inflight == 2 || v.inflight == 4)));
        default: return false;
    }
}

// A dense numbering of every (family, tag, flags) combination, built or not: launch_frame's
// table index and the variant part of the tile-schedule key.  5 flag bits: march and march_y
// shade, count, skip, gf, pipe; pair shade, gf, 4 lanes; mip and iso count, skip, log2(inflight)
// (2 bits); proj op, count, skip, log2(inflight).
constexpr int kVariantSlots = kVariantFamilies * kVariantTags * 32;
constexpr int variant_index(const FrameVariant &v)
{
    const int k = v.inflight == 1 ? 0 : v.inflight == 2 ? 1 : v.inflight == 4 ? 2 : 3;
    const bool march = v.family == VF_MARCH || v.family == VF_MARCH_Y;
    const int bits = march                 ? v.shade << 4 | v.count << 3 | v.skip << 2 | v.gf << 1 | (int)v.pipe
                     : v.family == VF_PAIR ? v.shade << 2 | v.gf << 1 | (v.lanes == 4)
                     : v.family == VF_PROJ ? (v.op == kProjMean) << 4 | v.count << 3 | v.skip << 2 | k
                                           : v.count << 3 | v.skip << 2 | k;
    return (v.family * kVariantTags + v.tag) * 32 + bits;
}
// Its inverse (a slot no variant maps to gives one that maps elsewhere or is not built).
constexpr FrameVariant variant_at(int i)
{
    const int family = i / 32 / kVariantTags, tag = i / 32 % kVariantTags;
    const auto bit = [i](int b) { return (i >> b & 1) != 0; };
    if (family == VF_MARCH || family == VF_MARCH_Y)
        return {family, tag, bit(4), bit(3), bit(2), bit(1), bit(0), 0, 0};
    if (family == VF_PAIR) return {family, tag, bit(2), false, false, bit(1), false, bit(0) ? 4 : 2, 0};
    return {family, tag, false, bit(3), bit(2), false, false, 0, (i & 3) == 3 ? 0 : 1 << (i & 3),
            family == VF_PROJ && bit(4) ? kProjMean : kProjMin};
}

// The demangled kernel name, as rocprofv3's kernel trace reports it ("Kernel_Name").
inline std::string variant_kernel_name(const FrameVariant &v)
{
    const auto b = [](bool x) { return x ? ", true" : ", false"; };
    if (v.family == VF_NONE || v.tag < 0 || v.tag >= kVariantTags) return "";
    const std::string ns = "void vr::(anonymous namespace)::", vt = kTagNames[v.tag];
    if (v.family == VF_MARCH)
        return ns + "march_kernel<" + vt + b(v.shade) + b(v.count) + b(v.skip) + b(v.gf) +
               b(v.pipe) + ">(vr::MarchParams)";
    if (v.family == VF_MARCH_Y)
        return ns + "march_y_kernel<" + vt + b(v.shade) + ">(vr::MarchParams)";
    if (v.family == VF_PAIR)
        return ns + "march_pair_kernel<" + vt + b(v.shade) + b(v.gf) + ", " +
               std::to_string(v.lanes) + ">(vr::MarchParams)";
    if (v.family == VF_PROJ)
        return ns + "proj_kernel<" + vt + ", " + std::to_string(v.op) + b(v.count) + b(v.skip) + ", " +
               std::to_string(v.inflight) + ">(vr::MarchParams, vr::ProjArgs)";
    return ns + (v.family == VF_ISO ? "iso_kernel<" : "mip_kernel<") + vt + b(v.count) + b(v.skip) +
           ", " + std::to_string(v.inflight) +
           (v.family == VF_ISO ? ">(vr::MarchParams, vr::IsoArgs)" : ">(vr::MarchParams, vr::MipArgs)");
}

// The adaptive tile order's schedule key: tile durations differ by kernel and by the copy it
// reads, so one variant's order is never learned from another's.
constexpr uint32_t variant_tile_key(const FrameVariant &v, int layout)
{
    static_assert(kVariantSlots <= 1 << 12, "the variant index and the layout would overlap");
    return (uint32_t)variant_index(v) | (uint32_t)layout << 12;
}

}  // namespace vr
