// RCCL, loaded on demand, and the observation gather over it: the only unit that knows librccl.
#include "rcw_handle.h"

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is loaded at run time (load_rccl)

#include <cstdlib>
#include <cstring>
#include <mutex>

namespace {

// ---- RCCL, loaded on demand ------------------------------------------------------------------------------
// librcw_hip does not link librccl: a single-GPU user never needs it, and inside a process that already
// carries one (PyTorch bundles its own copy under the same soname) a second instance must not be loaded.
// dlopen("librccl.so.1") returns the resident copy when there is one and the system one otherwise.
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
};
RcclApi g_rccl;

int load_rccl()
{
    // several handles of one process (one rank each, a thread each) may get here together: one loads, the others wait
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (g_rccl.lib) return RCW_OK;
    // RCW_RCCL_LIBRARY, where set, is THE library: one that cannot be loaded is an error, not a reason to fall back to another copy
    const char* const chosen = std::getenv("RCW_RCCL_LIBRARY");
    void* lib = nullptr;
    if (chosen && *chosen) {
        lib = dlopen(chosen, RTLD_NOW | RTLD_LOCAL);
        if (!lib) return fail(RCW_ERR_UNSUPPORTED, "RCW_RCCL_LIBRARY=%s could not be loaded (%s)", chosen, dlerror());
    } else {
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
    }
    if (!lib) return fail(RCW_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded (%s); set RCW_RCCL_LIBRARY", dlerror());
    RcclApi api;
    api.lib = lib;
#define RCW_SYM(field, name)                                                                       \
    api.field = reinterpret_cast<decltype(api.field)>(dlsym(lib, name));                          \
    if (!api.field) { dlclose(lib); return fail(RCW_ERR_UNSUPPORTED, "librccl lacks %s", name); }
    RCW_SYM(GetUniqueId, "ncclGetUniqueId")
    RCW_SYM(CommInitRank, "ncclCommInitRank")
    RCW_SYM(CommDestroy, "ncclCommDestroy")
    RCW_SYM(AllGather, "ncclAllGather")
    RCW_SYM(GroupStart, "ncclGroupStart")
    RCW_SYM(GroupEnd, "ncclGroupEnd")
    RCW_SYM(GetErrorString, "ncclGetErrorString")
    RCW_SYM(GetVersion, "ncclGetVersion")
#undef RCW_SYM
    g_rccl = api;
    return RCW_OK;
}

#define RCW_NCCL(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess) return fail(RCW_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

int need_comm(rcw_handle* h, const char* fn)
{
    if (!h->comm) return fail(RCW_ERR_INVALID_ARGUMENT, "%s: call rcw_comm_init first", fn);
    return RCW_OK;
}

}  // namespace

// ~rcw_handle's share of the communicator (its result is ignored: the handle goes either way)
void drop_comm(rcw_handle* h)
{
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy((ncclComm_t)h->comm);
}

extern "C" {

// ---- the observation gather (RCCL over xGMI) --------------------------------------------------------------
int rcw_comm_unique_id(void* out_id)
{
    if (!out_id) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    int rc = load_rccl(); if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == RCW_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    RCW_NCCL(g_rccl.GetUniqueId(&id));
    std::memcpy(out_id, &id, sizeof id);
    return RCW_OK;
}

int rcw_comm_init(rcw_handle* h, const void* unique_id, int32_t rank, int32_t world)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!unique_id || world < 1 || rank < 0 || rank >= world)
        return fail(RCW_ERR_INVALID_ARGUMENT, "bad rank %d / world %d", rank, world);
    if (h->comm) return fail(RCW_ERR_INVALID_ARGUMENT, "the handle already has a communicator (rcw_comm_destroy first)");
    rc = load_rccl(); if (rc) return rc;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    ncclComm_t comm = nullptr;
    RCW_NCCL(g_rccl.CommInitRank(&comm, world, id, rank));
    h->comm = comm; h->comm_rank = rank; h->comm_world = world;
    return RCW_OK;
}

int rcw_comm_destroy(rcw_handle* h)
{
    int rc = check_handle(h); if (rc) return rc;
    if (!h->comm) return RCW_OK;
    // the gathered-descriptor scratch is sized by the world: a later rcw_comm_init may have another (and the wait is the communicator's too)
    RCW_HIP(replace_buffers(h, {&h->d_gather_h, &h->d_gather_c}));
    RCW_NCCL(g_rccl.CommDestroy((ncclComm_t)h->comm));
    h->comm = nullptr; h->comm_rank = 0; h->comm_world = 0;
    return RCW_OK;
}

int rcw_comm_info(rcw_handle* h, int32_t* rank, int32_t* world)
{
    if (!h || !rank || !world) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    *rank = h->comm_rank; *world = h->comm_world;
    return RCW_OK;
}

int rcw_gather_columns(rcw_handle* h, int32_t* height_all, uint8_t* colour_all)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need_comm(h, "rcw_gather_columns"); if (rc) return rc;
    if (!height_all || !colour_all) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    rc = ensure_columns(h); if (rc) return rc;
    const size_t n = (size_t)h->B * h->cfg.num_rays;
    // one fused group: the two all-gathers progress together on the handle's stream, behind the step
    RCW_NCCL(g_rccl.GroupStart());
    ncclResult_t r1 = g_rccl.AllGather(h->d_col_h.get(), height_all, n, ncclInt32, (ncclComm_t)h->comm, h->stream);
    ncclResult_t r2 = g_rccl.AllGather(h->d_col_c.get(), colour_all, n, ncclUint8, (ncclComm_t)h->comm, h->stream);
    RCW_NCCL(g_rccl.GroupEnd());
    RCW_NCCL(r1); RCW_NCCL(r2);
    return RCW_OK;
}

int rcw_gather_observations(rcw_handle* h, int32_t mode, void* frames_all)
{
    int rc = check_handle(h); if (rc) return rc;
    rc = need_comm(h, "rcw_gather_observations"); if (rc) return rc;
    if (!frames_all) return fail(RCW_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((uintptr_t)frames_all & 15u) return fail(RCW_ERR_INVALID_ARGUMENT, "frames must be 16-byte aligned");
    const size_t N = (size_t)h->cfg.num_rays, Hc = (size_t)h->cfg.height_camera_view_pu;
    if (mode == RCW_GATHER_FRAMES) {
        RCW_NCCL(g_rccl.AllGather(h->dev.obs, frames_all, (size_t)h->B * N * Hc, ncclUint32, (ncclComm_t)h->comm, h->stream));
        return RCW_OK;
    }
    if (mode != RCW_GATHER_COLUMNS) return fail(RCW_ERR_INVALID_ARGUMENT, "unknown gather mode %d", mode);
    const size_t all = (size_t)h->B * h->comm_world;
    if ((long long)all > 0x7fffffffll) return fail(RCW_ERR_UNSUPPORTED, "global batch too large");
    if (!h->d_gather_h.get()) RCW_HIP(h->d_gather_h.hipMalloc(all * N * sizeof(int32_t)));
    if (!h->d_gather_c.get()) RCW_HIP(h->d_gather_c.hipMalloc(all * N));
    rc = rcw_gather_columns(h, h->d_gather_h.get<int32_t>(), h->d_gather_c.get<uint8_t>()); if (rc) return rc;
    RCW_HIP(rcw_launch_expand(h->dev, h->d_gather_h.get<int32_t>(), h->d_gather_c.get<uint8_t>(), (int32_t)all,
                              (uint32_t*)frames_all, h->stream));
    return RCW_OK;
}

}  // extern "C"
