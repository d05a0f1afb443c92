// Host pieces the two server rebuild calls share (server_rebuild_batch.hip: the CRebuild_Cached form, which defines them;
// server_rebuild_aligned_batch.hip: the CRebuild_No_Cached form): the workspace, the argument checks, and the front of the launch
// sequence -- everything up to the point where the two forms part.  (Shared with the other write batches: write_batch_host.hpp.)
#pragma once
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

namespace porla {

struct SrDesc;

struct ServerRebuildWs {
    std::mutex mu;
    int device = -1;
    Buf list, planes, work, work_y;
    Buf scalars;                  // the aligned form's rows of alignment scalars, one group of requests at a time
    PinnedList h_list;
    UseFence fence;
};

// what the front leaves for the rest of a call (device pointers into the workspace; work / work_y: K * n_total projective points)
struct SrFront {
    const SrDesc* d_desc;
    uint32_t* planes;
    size_t plane_words;
    void* work;
    void* work_y;
};

// the checks made before the device is touched (PORLA_ERR_ARG with a message naming `who`)
int sr_check(const char* who, const porla_server_rebuild_req* reqs, size_t k, size_t n_total, size_t n_cols, int curve);
// this device's workspace
int sr_workspace(ServerRebuildWs** out);
// ws->mu held, ws->fence entered: the descriptors' upload, the store, the passes of the data network but the last (their residue
// planes wait in F.planes; a network of one pass leaves nothing), the MAC load, the stages of the MAC network and the Y scaling,
// over all k requests.  The last data pass and the close are the caller's.
int sr_enqueue_front(ServerRebuildWs* ws, int curve, const porla_server_rebuild_req* reqs, size_t k, size_t n, size_t ncols, hipStream_t stream,
                     SrFront* F);

}  // namespace porla
