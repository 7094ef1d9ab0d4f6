// gallery_host.h -- rfd_gallery: what a face gallery (include/rfd.h, "gallery") owns on the device, next to the book of its rows
// (gallery_book.h).  gallery_host.hip holds every rfd_gallery_* entry; the kernels are kernels_gallery.hip.  Host only.
#pragma once
#include "ctx_access.h" // what a gallery needs of its context: ctx_stream, ctx_device
#include "gallery_book.h"
#include "host_resources.h"

// The enrolled embeddings of one context in HBM.  Next to the context, which lends it its device and stream; the caller destroys
// it first.
struct rfd_gallery {
    rfd_ctx *ctx = nullptr;
    rfd::GalleryBook book; // dim, capacity, rows, liveness, identities: the host's truth
    int groups_max = 0;    // workgroups of a search, from the CU count: the workspace holds their lists
    rfd::DevBuf store;     // ceil(capacity / 16) blocks of 16 rows, bf16, fragment-major (gallery_offset)
    rfd::DevBuf ws;        // [groups_max][32][RFD_GALLERY_MAX_K] keys
    // host forms, allocated by the first of them: a page-locked buffer and its device twin
    static constexpr size_t kStageBytes = 4u << 20;
    rfd::DevBuf stage;
    rfd::Pinned<char> pin;
    rfd::DevBuf live; // the device twin of the book's live words: ceil(capacity / 16) words, zero beyond book.unsynced().row0
    // row lists of remove / replace / set-identities / set-tags travel through a ring of page-locked slots (like the context's frame
    // descriptors), so the calls enqueue without waiting for the stream; allocated by the first such call.  A slot is laid out
    // by the book (kEditInts).
    static constexpr int kRing = 4;
    rfd::PinnedRing<kRing> edit_ring;
    rfd::DevBuf edit;
    // The identities on the device (one int32 per row, in whole blocks of 16; -1 = unlabelled), allocated by the first
    // rfd_gallery_set_identities; until then no call touches them and every search runs without them.
    rfd::DevBuf ids;
    // The tags on the device (one uint32 per row, in whole blocks of 16, zero for every row without one), allocated by the first
    // rfd_gallery_set_tags or the first filtered search; until then no call touches them, and the plain and the identity
    // searches never do.
    rfd::DevBuf tags;
    // The workspace of rfd_gallery_nearest (rfd.h, "nearest"): the splits' keys, sized once for any call on this gallery
    // (gallery_nearest_ws_bound) by the first such call, so it never moves under enqueued work.
    int cus = 0; // of the gallery's device, from creation
    rfd::DevBuf nearest_ws;
};
