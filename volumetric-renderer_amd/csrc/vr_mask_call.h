// vr_mask_call.h — private to csrc/vr_api_{morph,maskcc,mstat,mview,mmesh}.hip: what the entry points of the mask
// families share on top of vr_ctx.h -- the skeleton of an entry point with an info struct
// (mask_call), the host forms' staging of their arrays in device memory (MaskStage) and the
// family's last kernel name.  The request checks it runs are vr_mask_host.h's and the family's.
#pragma once

#include "vr_ctx.h"
#include "vr_mask_host.h"

#include <type_traits>

namespace vr {

static_assert(VR_OK == kMaskOk && VR_EINVAL == kMaskEinval && VR_ENOSPC == kMaskEnospc, "vr_mask_host.h");

inline int null_ctx() { return fail(nullptr, VR_EINVAL, "ctx is NULL"); }

// An entry point with an info struct, whose first field is the grid's voxels.  In this order:
//   a NULL context is refused;
//   check(&msg) is the family's request check: VR_OK or VR_ENOSPC with g resolved, or VR_EINVAL,
//     which fails;
//   a multi-device context hands the call to its replica: reenter(m) is the entry point on member m;
//   admit(), where the family has one (not nullptr), checks what needs the member's volume;
//   body(&I) runs the passes, and *info = I on VR_OK only.
// VR_ENOSPC is reported, with *info = {g.voxels} and every other field 0 (all the host knows), as
// soon as everything that outranks it is checked: after admit(), whose VR_EINVAL outranks it and
// which needs the member, or straight after the check in a family without one.
template <class Info, class Check, class Reenter, class Admit, class Body>
int mask_call(vr_ctx *c, const MaskGrid &g, Info *info, Check check, Reenter reenter, Admit admit, Body body)
{
    constexpr bool admits = !std::is_null_pointer<Admit>::value;
    if (!c) return null_ctx();
    const char *msg;
    const int rc = check(&msg);
    auto refuse = [&] {
        if (rc == VR_ENOSPC) *info = Info{g.voxels};
        return fail(c, rc, msg);
    };
    if (rc == VR_EINVAL || (rc && !admits)) return refuse();
    if (is_group(c)) return on_replica(c, reenter);
    if constexpr (admits)
        if (int rc2 = admit()) return rc2;
    if (rc) return refuse();
    Info I;
    if (int rc2 = body(&I)) return rc2;
    *info = I;
    return VR_OK;
}

// The host forms' copies in device memory: up to two inputs from the start of block b in order,
// the result of out_bytes behind them, each 8-byte aligned.  An input whose host pointer is NULL is
// absent (in[i] stays NULL); one of 0 bytes keeps its place and is not copied.
struct MaskInput {
    const void *host;
    size_t bytes;
    const char *what;  // names the copy in an error
};

struct MaskStage {
    vr_ctx *c;
    char *in[2] = {nullptr, nullptr}, *out = nullptr;
    size_t out_bytes = 0;

    int begin(DevBlock &b, const char *what, const char *idle_first, MaskInput a, MaskInput a2, size_t result_bytes)
    {
        HIP_TRY(c, hipSetDevice(c->device), "hipSetDevice");
        const MaskInput ins[2] = {a, a2};
        size_t off[3] = {0, 0, 0};
        for (int i = 0; i < 2; ++i) off[i + 1] = off[i] + (((ins[i].host ? ins[i].bytes : 0) + 7) & ~(size_t)7);
        if (int rc = reserve(c, b, off[2] + result_bytes, what, idle_first)) return rc;
        char *io = static_cast<char *>(b.p);
        for (int i = 0; i < 2; ++i) {
            if (!ins[i].host) continue;
            in[i] = io + off[i];
            if (ins[i].bytes) HIP_TRY(c, hipMemcpy(in[i], ins[i].host, ins[i].bytes, hipMemcpyHostToDevice), ins[i].what);
        }
        out = io + off[2];
        out_bytes = result_bytes;
        return VR_OK;
    }
    // the result to the host
    int finish(void *host, const char *what)
    {
        HIP_TRY(c, hipMemcpy(host, out, out_bytes, hipMemcpyDeviceToHost), what);
        return VR_OK;
    }
};

// vr_<family>_last_kernel_name: the member's (the replica's, on a multi-device context).
inline const char *mask_last_kernel_name(const vr_ctx *c, const char *vr_ctx::*name)
{
    if (!c) return "";
    return (is_group(c) ? c->members[0] : c)->*name;
}

}  // namespace vr
