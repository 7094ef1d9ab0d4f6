// face_host.h -- what the face stage (include/rfd.h: selection, alignment, model inputs, the packed face list, the quality and
// normalisation rules, liveness) keeps in a context.  face_host.hip holds every entry from rfd_selection_config_default to
// rfd_liveness_decide; the kernels are kernels_pre.hip and kernels_post.hip (kernels.h); the checks, the splits and the layouts
// of the staging buffers are face_plan.h.
#pragma once
#include "ctx_access.h"
#include "face_plan.h"
#include "kernels.h"

namespace rfd {

// The part of a context that belongs to the face stage.  Every buffer grows on demand and is reused by the next call in
// stream order, whichever entry that is; the rings but dims_ring are allocated by the first call that needs them.
struct FaceStage {
    // selection: the frame sizes of its epilogue, and the selection of the host-output entries (SelLayout)
    DevBuf sel_dims, sel_out;
    // alignment: the set-up records, and crops and status of the host-output entries
    DevBuf align_faces, align_out, align_status;
    // model inputs of the quality / ID stages: staged crops and per-config planes of the host entries; in / out staging of the
    // host forms of the decision rule and the normalisation
    DevBuf face_in, face_tensors[kMaxFaceTensors], face_io[2];
    // packed face list of the host-output entries (ListLayout), and the page-locked copy of total | first [B + 1] that tells
    // the host how many rows to fetch
    DevBuf list_out;
    Pinned<int> h_list;
    // Per-call descriptors travel through rings of page-locked slots, so enqueueing never blocks on the previous call.
    static constexpr int kRing = 4;
    PinnedRing<kRing> dims_ring; // frame sizes of the selection epilogue: h i32 [n] | w i32 [n]; allocated with the context
    PinnedRing<kRing> live_ring; // LiveImage [B]
    // liveness: frame descriptors, the per-(face, model) geometry, the in / out staging of the host forms (LiveTensorLayout,
    // LiveDecideLayout), the running sums of a decide call of many models
    DevBuf live_imgs, live_geo, live_io, live_acc;
};

} // namespace rfd
