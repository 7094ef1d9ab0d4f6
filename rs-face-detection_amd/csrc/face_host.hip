// face_host.hip -- the face stage of include/rfd.h behind the detection: selection, alignment, the model inputs of the quality
// and ID stages, the packed face list, the quality and normalisation rules, liveness.  What a context keeps for them is
// face_host.h (FaceStage), what they decide on the host is face_plan.h, what they ask of the context is ctx_access.h; the kernels
// are those of kernels.h.
#include "face_host.h"

#include <algorithm>
#include <vector>

using namespace rfd;

// a check of face_plan.h; its refusal is the call's error
#define RFD_PLAN(check, ...)                                   \
    do {                                                       \
        char _msg[192];                                        \
        const int _s = check(__VA_ARGS__, _msg, sizeof _msg);  \
        if (_s != RFD_OK) {                                    \
            ::rfd::set_error("%s", _msg);                      \
            return _s;                                         \
        }                                                      \
    } while (0)

namespace {

// the end of an entry whose results the caller reads: enqueued only (async), or waited for, and then no device-side wait gave up
int finish(rfd_ctx *c, int async = 0)
{
    if (async) return RFD_OK;
    RFD_HIP(hipStreamSynchronize(ctx_stream(c)));
    return ctx_check_nms_flag(c);
}

// the sizes of n frames as the selection takes them
struct FrameSizes {
    std::vector<int> h, w;
    FrameSizes(const rfd_image *imgs, int n) : h(n), w(n)
    {
        for (int i = 0; i < n; ++i) { h[i] = imgs[i].height; w[i] = imgs[i].width; }
    }
};

// bytes of one face's planes [3][out_h][out_w] f32 of every model input of a call
struct PlaneBytes { size_t of[kMaxFaceTensors]; };
PlaneBytes plane_bytes(const rfd_face_tensor_config *cfgs, int k)
{
    PlaneBytes b = {};
    for (int j = 0; j < k; ++j) b.of[j] = (size_t)3 * cfgs[j].out_w * cfgs[j].out_h * sizeof(float);
    return b;
}
PlaneBytes plane_bytes(const rfd_liveness_config &cfg)
{
    PlaneBytes b = {};
    for (int j = 0; j < cfg.k; ++j) b.of[j] = (size_t)3 * cfg.out_w[j] * cfg.out_h[j] * sizeof(float);
    return b;
}

// the context's own planes of k model inputs for `faces` faces, into d [k]
int own_planes(FaceStage &fs, size_t faces, int k, const PlaneBytes &b, float **d)
{
    for (int j = 0; j < k; ++j) {
        RFD_TRY(fs.face_tensors[j].reserve(faces * b.of[j]));
        d[j] = (float *)fs.face_tensors[j].p;
    }
    return RFD_OK;
}

// ---- selection ----
// selection over device-resident detection slabs into device arrays d_box [n][5], d_kps [n][10], d_found [n]; enqueued only.
// The frame sizes go through a ring of page-locked arrays (as the frame descriptors do), so nothing here needs the host to
// wait for the stream.
int select_enqueue(rfd_ctx *c, const rfd_dets &dets, const int *img_h, const int *img_w, int n, const rfd_selection_config *cfg,
                   int is_enroll, float *d_box, float *d_kps, int32_t *d_found)
{
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    rfd_selection_config def;
    selection_config_default(&def);
    if (!cfg) cfg = &def;
    RFD_TRY(fs.sel_dims.reserve((size_t)2 * n * sizeof(int)));
    int *dims;
    RFD_TRY(fs.dims_ring.acquire(&dims));
    for (int i = 0; i < n; ++i) { dims[i] = img_h[i]; dims[n + i] = img_w[i]; }
    RFD_HIP(hipMemcpyAsync(fs.sel_dims.p, dims, 2 * n * sizeof(int), hipMemcpyHostToDevice, s));
    RFD_TRY(fs.dims_ring.record(s));
    SelectParams sp;
    memset(&sp, 0, sizeof sp);
    sp.boxes = dets.boxes; sp.lmk = dets.landmarks; sp.count = dets.count;
    sp.img_h = (const int *)fs.sel_dims.p; sp.img_w = sp.img_h + n;
    sp.n = n; sp.max_det = ctx_max_det(c); sp.is_enroll = is_enroll;
    sp.margin_center_left_ratio = cfg->margin_center_left_ratio;
    sp.margin_center_right_ratio = cfg->margin_center_right_ratio;
    sp.margin_edge_ratio = cfg->margin_edge_ratio;
    sp.minimum_face_ratio = cfg->minimum_face_ratio;
    sp.out_box = d_box; sp.out_kps = d_kps; sp.out_found = d_found;
    return launch_face_select(sp, s);
}

// the selection of n frames in the context's own buffer (SelLayout)
struct SelView { float *box, *kps; int32_t *found; };
int sel_own(FaceStage &fs, int n, SelView *v)
{
    const SelLayout l = sel_layout(n);
    RFD_TRY(fs.sel_out.reserve(l.words * 4));
    float *o = (float *)fs.sel_out.p;
    *v = SelView{o + l.box, o + l.kps, (int32_t *)(o + l.found)};
    return RFD_OK;
}

// a selection the caller holds on the host, into the own buffer
int sel_upload(rfd_ctx *c, int n, const float *boxes, const float *kps, const int32_t *found, SelView *v)
{
    const hipStream_t s = ctx_stream(c);
    RFD_TRY(sel_own(ctx_face_stage(c), n, v));
    RFD_HIP(hipMemcpyAsync(v->box, boxes, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_HIP(hipMemcpyAsync(v->kps, kps, (size_t)n * 10 * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_HIP(hipMemcpyAsync(v->found, found, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    return RFD_OK;
}

// select_enqueue into the own buffer, then copied to the host pointers
int select_impl(rfd_ctx *c, const rfd_dets &dets, const int *img_h, const int *img_w, int n, const rfd_selection_config *cfg,
                int is_enroll, float *out_box, float *out_kps, int32_t *found)
{
    const hipStream_t s = ctx_stream(c);
    SelView v;
    RFD_TRY(sel_own(ctx_face_stage(c), n, &v));
    RFD_TRY(select_enqueue(c, dets, img_h, img_w, n, cfg, is_enroll, v.box, v.kps, v.found));
    RFD_HIP(hipMemcpyAsync(out_box, v.box, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(out_kps, v.kps, (size_t)n * 10 * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(found, v.found, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    return finish(c); // the results are read by the caller
}

// rfd_detect_select_batch; *staged: the descriptors of the frames, which stay staged until the next call on this context
int detect_select(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_selection_config *cfg, int is_enroll, float *out_box,
                  float *out_kps, int32_t *found, const PreImage **staged)
{
    RFD_CHECK_ARG(c && out_box && out_kps && found, "null argument");
    RFD_TRY(ctx_check_images(c, imgs, n));
    rfd_dets dev;
    RFD_TRY(ctx_detect_own_slabs(c, imgs, n, /*frames on device*/ false, &dev, staged));
    const FrameSizes sz(imgs, n);
    return select_impl(c, dev, sz.h.data(), sz.w.data(), n, cfg, is_enroll, out_box, out_kps, found);
}

// ---- alignment and model inputs ----
// the caller's alignment config or, for null, the reference's (into *def); refused if its output size is out of range
int resolve_align_cfg(const rfd_alignment_config **cfg, rfd_alignment_config *def)
{
    if (!*cfg) { alignment_config_default(def); *cfg = def; }
    RFD_PLAN(check_align_cfg, **cfg);
    return RFD_OK;
}

// The faces a launch works on.  One per frame: face b is frame b, found [n] says what the selection holds of it.  Or a packed
// list: face t reads frame frame[t], found is null (a listed face has box and key points), n is the host-known bound of the
// launch and every face past min(*total, cap) leaves its rows alone.
struct Faces {
    int n;
    const float *box, *kps;
    const int32_t *found;
    const int32_t *frame, *total;
    int cap;
};

// where a launch writes: crops (may be null), status, the k model inputs
struct FaceOut {
    uint8_t *crops;
    int32_t *status;
    float *const *tensors;
};

// what the aligners need: the staged frames, the faces, the template, the set-up records, the outputs
int align_params(FaceStage &fs, const PreImage *frames, const Faces &f, const rfd_alignment_config &cfg, uint8_t *crops,
                 int32_t *status, AlignParams *ap)
{
    RFD_TRY(fs.align_faces.reserve((size_t)f.n * sizeof(AlignFace)));
    memset(ap, 0, sizeof *ap);
    ap->imgs = frames;
    ap->box = f.box; ap->kps = f.kps; ap->found = f.found;
    memcpy(ap->std_lmk, cfg.standard_landmarks, sizeof ap->std_lmk);
    ap->out_w = cfg.out_w; ap->out_h = cfg.out_h; ap->n = f.n;
    ap->faces = (AlignFace *)fs.align_faces.p;
    ap->status = status;
    ap->out = crops;
    ap->frame = f.frame; ap->total = f.total; ap->cap = f.cap;
    return RFD_OK;
}

// alignment of one selected face per staged frame; crops and status are copied to the host pointers
int align_impl(rfd_ctx *c, const PreImage *frames, int n, const SelView &v, const rfd_alignment_config *cfg, uint8_t *out_crops,
               int32_t *status)
{
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    rfd_alignment_config def;
    RFD_TRY(resolve_align_cfg(&cfg, &def));
    const size_t crop = (size_t)cfg->out_w * cfg->out_h * 3;
    RFD_TRY(fs.align_out.reserve((size_t)n * crop));
    RFD_TRY(fs.align_status.reserve((size_t)n * sizeof(int)));
    AlignParams ap;
    RFD_TRY(align_params(fs, frames, Faces{n, v.box, v.kps, v.found, nullptr, nullptr, 0}, *cfg, (uint8_t *)fs.align_out.p,
                         (int32_t *)fs.align_status.p, &ap));
    RFD_TRY(launch_face_align(ap, s));
    RFD_HIP(hipMemcpyAsync(out_crops, ap.out, (size_t)n * crop, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(status, ap.status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    return finish(c);
}

int check_face_tensor_args(const rfd_face_tensor_config *cfgs, int k, float *const *tensors, int k_min)
{
    RFD_PLAN(check_face_tensor_count, k, k_min);
    RFD_CHECK_ARG(k == 0 || (cfgs && tensors), "tensor configs / tensor pointers are null");
    for (int j = 0; j < k; ++j) {
        RFD_PLAN(check_face_tensor_size, cfgs[j], j);
        if (!tensors[j]) { set_error("tensor pointer %d is null", j); return RFD_ERR_INVALID_ARG; }
    }
    return RFD_OK;
}

void fill_face_tensor_cfg(FaceTensorCfg &d, const rfd_face_tensor_config &s, float *out, int crop_w, int crop_h)
{
    d.out = out; d.out_w = s.out_w; d.out_h = s.out_h;
    memcpy(d.mean, s.mean, sizeof d.mean);
    memcpy(d.scale, s.scale, sizeof d.scale);
    d.same = s.out_w == crop_w && s.out_h == crop_h;
    const ResizeScale r = resize_scale(crop_w, crop_h, s.out_w, s.out_h);
    d.scale_x = r.scale_x; d.scale_y = r.scale_y; d.area_fast = r.area_fast;
}

// Set-up, warp and the k model inputs of every face of f on the staged frames, into DEVICE arrays; enqueued only.  Configs of
// the crop's own size are written by the warp itself; the others are resized from the crop in HBM (out.crops, or the context's
// own buffer when the caller wants no crop).
int align_tensors_enqueue(rfd_ctx *c, const PreImage *frames, const Faces &f, const rfd_alignment_config &cfg,
                          const rfd_face_tensor_config *cfgs, int k, const FaceOut &out)
{
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const FaceSplit split = face_split(cfg.out_w, cfg.out_h, cfgs, k);
    FaceTensorParams fused, rest;
    memset(&fused, 0, sizeof fused);
    memset(&rest, 0, sizeof rest);
    for (int q = 0; q < split.n_fused; ++q)
        fill_face_tensor_cfg(fused.cfg[fused.k++], cfgs[split.fused[q]], out.tensors[split.fused[q]], cfg.out_w, cfg.out_h);
    for (int q = 0; q < split.n_rest; ++q)
        fill_face_tensor_cfg(rest.cfg[rest.k++], cfgs[split.rest[q]], out.tensors[split.rest[q]], cfg.out_w, cfg.out_h);
    uint8_t *crops = out.crops;
    if (!crops && rest.k) {
        RFD_TRY(fs.align_out.reserve((size_t)f.n * cfg.out_w * cfg.out_h * 3));
        crops = (uint8_t *)fs.align_out.p;
    }
    AlignParams ap;
    RFD_TRY(align_params(fs, frames, f, cfg, crops, out.status, &ap));
    fused.n = rest.n = f.n;
    fused.crop_w = rest.crop_w = cfg.out_w;
    fused.crop_h = rest.crop_h = cfg.out_h;
    rest.crops = crops;
    rest.status = out.status;
    rest.total = f.total; rest.cap = f.cap;
    RFD_TRY(launch_face_align_tensors(ap, fused, s));
    return launch_face_tensors(rest, s);
}

// align_tensors_enqueue on the selection results in the own buffer, into the context's own buffers, then copied to the host
// pointers
int align_tensors_to_host(rfd_ctx *c, const PreImage *frames, int n, const rfd_alignment_config *align_cfg, uint8_t *out_crops,
                          int32_t *status, const rfd_face_tensor_config *cfgs, int k, float *const *tensors)
{
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t crop = (size_t)align_cfg->out_w * align_cfg->out_h * 3;
    RFD_TRY(fs.align_status.reserve((size_t)n * sizeof(int)));
    if (out_crops) RFD_TRY(fs.align_out.reserve((size_t)n * crop));
    const PlaneBytes planes = plane_bytes(cfgs, k);
    float *d_tensors[kMaxFaceTensors] = {};
    RFD_TRY(own_planes(fs, n, k, planes, d_tensors));
    SelView v;
    RFD_TRY(sel_own(fs, n, &v));
    RFD_TRY(align_tensors_enqueue(c, frames, Faces{n, v.box, v.kps, v.found, nullptr, nullptr, 0}, *align_cfg, cfgs, k,
                                  FaceOut{out_crops ? (uint8_t *)fs.align_out.p : nullptr, (int32_t *)fs.align_status.p, d_tensors}));
    if (out_crops) RFD_HIP(hipMemcpyAsync(out_crops, fs.align_out.p, (size_t)n * crop, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(status, fs.align_status.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
    for (int j = 0; j < k; ++j) RFD_HIP(hipMemcpyAsync(tensors[j], d_tensors[j], n * planes.of[j], hipMemcpyDeviceToHost, s));
    return finish(c);
}

// ---- every detected face of a frame: the packed face list (rfd.h) ----
// the caller's list config or, for null, the default (into *def)
int resolve_list_cfg(const rfd_face_list_config **cfg, rfd_face_list_config *def, int cap)
{
    if (!*cfg) { face_list_config_default(def); *cfg = def; }
    RFD_PLAN(check_list_cfg, **cfg, cap);
    return RFD_OK;
}

// The list of the detections in the device slabs `dets` of the n staged frames, then set-up, warp and tensors over it, all
// into the DEVICE arrays of `out`; enqueued only.
int face_list_enqueue(rfd_ctx *c, const PreImage *frames, int n, const rfd_dets &dets, const rfd_face_list_config *lc,
                      const rfd_alignment_config *cfg, const rfd_face_tensor_config *cfgs, int k, int cap, const rfd_face_list &out)
{
    FaceListParams lp;
    memset(&lp, 0, sizeof lp);
    lp.boxes = dets.boxes; lp.lmk = dets.landmarks; lp.count = dets.count;
    lp.n = n; lp.max_det = ctx_max_det(c); lp.max_faces = lc->max_faces; lp.cap = cap;
    lp.min_face_px = lc->min_face_px; lp.min_score = lc->min_score;
    lp.total = out.total; lp.first = out.first; lp.frame = out.frame; lp.row = out.row; lp.box = out.box; lp.kps = out.kps;
    RFD_TRY(launch_face_list(lp, ctx_stream(c)));
    const int bound = face_list_bound(n, lc->max_faces, ctx_max_det(c), cap);
    return align_tensors_enqueue(c, frames, Faces{bound, out.box, out.kps, nullptr, out.frame, out.total, cap}, *cfg, cfgs, k,
                                 FaceOut{out.crops, out.status, out.tensors});
}

// the list of a host-output call in the context's own buffers (ListLayout)
int face_list_own(rfd_ctx *c, int n, int bound, const rfd_alignment_config *cfg, const PlaneBytes &planes, int k, bool want_crops,
                  rfd_face_list *v)
{
    FaceStage &fs = ctx_face_stage(c);
    const ListLayout l = list_layout(n, bound);
    RFD_TRY(fs.list_out.reserve(l.words * 4));
    RFD_TRY(fs.h_list.alloc((size_t)ctx_max_batch_size(c) + 2));
    memset(v, 0, sizeof *v);
    int32_t *o = (int32_t *)fs.list_out.p;
    v->total = o + l.total; v->first = o + l.first;
    v->frame = o + l.frame; v->row = o + l.row; v->status = o + l.status;
    v->box = (float *)(o + l.box); v->kps = (float *)(o + l.kps);
    if (want_crops) {
        RFD_TRY(fs.align_out.reserve((size_t)bound * cfg->out_w * cfg->out_h * 3));
        v->crops = (uint8_t *)fs.align_out.p;
    }
    return own_planes(fs, bound, k, planes, v->tensors);
}

// face_list_enqueue into the context's own buffers, then to the host pointers of `out`: the stream is waited for once, for
// total and first, and only the min(T, cap) listed rows are fetched after it -- the caller's rows past them stay as they are.
int face_list_to_host(rfd_ctx *c, const PreImage *frames, int n, const rfd_dets &dets, const rfd_face_list_config *lc,
                      const rfd_alignment_config *cfg, const rfd_face_tensor_config *cfgs, int k, int cap, rfd_face_list *out)
{
    FaceStage &fs = ctx_face_stage(c);
    const PlaneBytes planes = plane_bytes(cfgs, k);
    rfd_face_list v;
    RFD_TRY(face_list_own(c, n, face_list_bound(n, lc->max_faces, ctx_max_det(c), cap), cfg, planes, k, out->crops != nullptr, &v));
    RFD_TRY(face_list_enqueue(c, frames, n, dets, lc, cfg, cfgs, k, cap, v));
    RFD_HIP(hipMemcpyAsync(fs.h_list, v.total, ((size_t)n + 2) * sizeof(int), hipMemcpyDeviceToHost, ctx_stream(c)));
    RFD_TRY(finish(c));
    out->total[0] = fs.h_list[0];
    memcpy(out->first, fs.h_list + 1, ((size_t)n + 1) * sizeof(int));
    const size_t rows = (size_t)std::min(fs.h_list[0], cap);
    if (!rows) return RFD_OK;
    RFD_HIP(hipMemcpy(out->frame, v.frame, rows * sizeof(int), hipMemcpyDeviceToHost));
    RFD_HIP(hipMemcpy(out->row, v.row, rows * sizeof(int), hipMemcpyDeviceToHost));
    RFD_HIP(hipMemcpy(out->status, v.status, rows * sizeof(int), hipMemcpyDeviceToHost));
    RFD_HIP(hipMemcpy(out->box, v.box, rows * 5 * sizeof(float), hipMemcpyDeviceToHost));
    RFD_HIP(hipMemcpy(out->kps, v.kps, rows * 10 * sizeof(float), hipMemcpyDeviceToHost));
    if (out->crops) RFD_HIP(hipMemcpy(out->crops, v.crops, rows * cfg->out_w * cfg->out_h * 3, hipMemcpyDeviceToHost));
    for (int j = 0; j < k; ++j) RFD_HIP(hipMemcpy(out->tensors[j], v.tensors[j], rows * planes.of[j], hipMemcpyDeviceToHost));
    return RFD_OK;
}

// the argument checks the four list entries share
int check_face_list_call(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_face_list_config **lc, rfd_face_list_config *ldef,
                         const rfd_alignment_config **ac, rfd_alignment_config *adef, const rfd_face_tensor_config *cfgs, int k,
                         int cap, const rfd_face_list *out)
{
    RFD_CHECK_ARG(c != nullptr, "ctx is null");
    RFD_CHECK_ARG(out && out->total && out->first && out->frame && out->row && out->box && out->kps && out->status,
                  "face list output pointers are null");
    RFD_TRY(check_face_tensor_args(cfgs, k, out->tensors, 0));
    RFD_TRY(resolve_list_cfg(lc, ldef, cap));
    RFD_TRY(resolve_align_cfg(ac, adef));
    return ctx_check_images(c, imgs, n);
}

// ---- quality rule, normalisation, liveness ----
int check_quality_args(const rfd_ctx *c, const float *logits, int n, int classes, const float *score, const int32_t *klass)
{
    RFD_CHECK_ARG(c && logits && score && klass, "null argument");
    RFD_PLAN(check_quality_counts, n, classes);
    return RFD_OK;
}

int check_normalize_args(const rfd_ctx *c, const float *emb, int n, int dim, const float *out)
{
    RFD_CHECK_ARG(c && emb && out, "null argument");
    RFD_PLAN(check_normalize_counts, n, dim);
    return RFD_OK;
}

// Both kernels of the tensor call on DEVICE boxes / flags into DEVICE outputs; enqueued only.  The frame descriptors go
// through a ring of page-locked arrays, so nothing here waits for the stream; host frames are staged first.
int liveness_enqueue(rfd_ctx *c, const rfd_image *imgs, int n, bool frames_on_device, const float *d_box, const int *d_found,
                     const rfd_liveness_config *cfg, float *const *d_tensors, float *d_weights, int32_t *d_rois, int32_t *d_status)
{
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t B = (size_t)ctx_max_batch_size(c);
    RFD_TRY(fs.live_ring.ensure(B * sizeof(LiveImage))); // first call on this context
    RFD_TRY(fs.live_imgs.reserve(B * sizeof(LiveImage)));
    RFD_TRY(fs.live_geo.reserve(B * kMaxFaceTensors * sizeof(LiveRoi)));
    LiveImage *li;
    RFD_TRY(fs.live_ring.acquire(&li));
    for (int i = 0; i < n; ++i) { li[i].h = imgs[i].height; li[i].w = imgs[i].width; }
    RFD_TRY(ctx_place_frames(c, imgs, n, frames_on_device, li, sizeof(LiveImage)));
    RFD_HIP(hipMemcpyAsync(fs.live_imgs.p, li, n * sizeof(LiveImage), hipMemcpyHostToDevice, s));
    RFD_TRY(fs.live_ring.record(s));
    const LiveTiles tiles = live_tiles(*cfg);
    LiveParams p;
    memset(&p, 0, sizeof p);
    p.imgs = (const LiveImage *)fs.live_imgs.p;
    p.box = d_box; p.found = d_found;
    p.n = n; p.k = cfg->k; p.tiles = tiles.total;
    for (int j = 0; j < cfg->k; ++j) {
        p.cfg[j].out = d_tensors[j]; p.cfg[j].scale = cfg->scale[j];
        p.cfg[j].out_w = cfg->out_w[j]; p.cfg[j].out_h = cfg->out_h[j];
        p.cfg[j].tile0 = tiles.tile0[j];
    }
    p.geo = (LiveRoi *)fs.live_geo.p;
    p.weights = d_weights; p.rois = d_rois; p.status = d_status;
    return launch_liveness_tensors(p, s);
}

int check_liveness_args(rfd_ctx *c, const rfd_image *imgs, int n, const float *boxes, const int32_t *found,
                        const rfd_liveness_config **cfg, rfd_liveness_config *def, float *const *tensors, const float *weights,
                        const int32_t *status)
{
    RFD_CHECK_ARG(c && boxes && found && tensors && weights && status, "null argument");
    if (!*cfg) { liveness_config_default(def); *cfg = def; }
    RFD_PLAN(check_liveness_cfg, **cfg);
    for (int j = 0; j < (*cfg)->k; ++j)
        if (!tensors[j]) { set_error("invalid argument: tensor pointer %d is null", j); return RFD_ERR_INVALID_ARG; }
    return ctx_check_images(c, imgs, n);
}

int check_liveness_decide_args(const rfd_ctx *c, const float *const *logits, int k, int n, int classes, const float *weights,
                               const float *score, const int32_t *live)
{
    RFD_CHECK_ARG(c && logits && weights && score && live, "null argument");
    RFD_PLAN(check_liveness_decide_counts, k, n, classes);
    for (int j = 0; j < k; ++j)
        if (!logits[j]) { set_error("invalid argument: logits pointer %d is null", j); return RFD_ERR_INVALID_ARG; }
    return RFD_OK;
}

} // namespace

// ================================================================================================
// C ABI
// ================================================================================================
void rfd_selection_config_default(rfd_selection_config *cfg) { if (cfg) selection_config_default(cfg); }
void rfd_alignment_config_default(rfd_alignment_config *cfg) { if (cfg) alignment_config_default(cfg); }
void rfd_face_tensor_config_quality(rfd_face_tensor_config *cfg) { if (cfg) face_tensor_config_quality(cfg); }
void rfd_face_tensor_config_extraction(rfd_face_tensor_config *cfg) { if (cfg) face_tensor_config_extraction(cfg); }
void rfd_face_tensor_config_quality_assessment(rfd_face_tensor_config *cfg, int w, int h) { if (cfg) face_tensor_config_quality_assessment(cfg, w, h); }
void rfd_face_list_config_default(rfd_face_list_config *cfg) { if (cfg) face_list_config_default(cfg); }
void rfd_liveness_config_default(rfd_liveness_config *cfg) { if (cfg) liveness_config_default(cfg); }

int rfd_select_faces(rfd_ctx *c, const rfd_dets *dets, const int *img_h, const int *img_w, int n,
                     const rfd_selection_config *cfg, int is_enroll, float *out_box, float *out_kps, int32_t *found)
{
    RFD_CHECK_ARG(c && dets && dets->boxes && dets->landmarks && dets->count && img_h && img_w && out_box && out_kps && found,
                  "null argument");
    RFD_TRY(ctx_check_batch(c, n, "batch"));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    rfd_dets dev = ctx_own_slabs(c);
    dev.total = nullptr; // the selection does not read it
    RFD_TRY(ctx_copy_slabs(c, dev, *dets, n, hipMemcpyHostToDevice));
    return select_impl(c, dev, img_h, img_w, n, cfg, is_enroll, out_box, out_kps, found);
}

int rfd_detect_select_batch(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_selection_config *cfg, int is_enroll,
                            float *out_box, float *out_kps, int32_t *found)
{
    const PreImage *frames;
    return detect_select(c, imgs, n, cfg, is_enroll, out_box, out_kps, found, &frames);
}

int rfd_align_faces(rfd_ctx *c, const rfd_image *imgs, int n, const float *boxes, const float *kps, const int32_t *found,
                    const rfd_alignment_config *cfg, uint8_t *out_crops, int32_t *status)
{
    RFD_CHECK_ARG(c && boxes && kps && found && out_crops && status, "null argument");
    RFD_TRY(ctx_check_images(c, imgs, n));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const PreImage *frames;
    RFD_TRY(ctx_stage_frames(c, imgs, n, false, &frames));
    SelView v;
    RFD_TRY(sel_upload(c, n, boxes, kps, found, &v));
    return align_impl(c, frames, n, v, cfg, out_crops, status);
}

// the set-up records of n faces on frames of which only the sizes exist: descriptors without pixels, then the set-up launch of
// align_impl
int rfd_debug_align_setup(rfd_ctx *c, int n, const float *boxes, const float *kps, const int32_t *found, const int32_t *img_w,
                          const int32_t *img_h, const rfd_alignment_config *cfg, int32_t *mode, double *M, int32_t *roi,
                          double *scale, int32_t *area_fast)
{
    RFD_CHECK_ARG(c && boxes && kps && found && img_w && img_h && mode && M && roi && scale && area_fast, "null argument");
    RFD_TRY(ctx_check_batch(c, n, "batch of", " faces"));
    rfd_alignment_config def;
    RFD_TRY(resolve_align_cfg(&cfg, &def));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const PreImage *frames;
    RFD_TRY(ctx_stage_frame_sizes(c, img_w, img_h, n, &frames));
    SelView v;
    RFD_TRY(sel_upload(c, n, boxes, kps, found, &v));
    RFD_TRY(fs.align_status.reserve((size_t)n * sizeof(int)));
    AlignParams ap;
    RFD_TRY(align_params(fs, frames, Faces{n, v.box, v.kps, v.found, nullptr, nullptr, 0}, *cfg, nullptr, (int32_t *)fs.align_status.p, &ap));
    RFD_TRY(launch_face_align_setup(ap, s));
    std::vector<AlignFace> faces(n);
    RFD_HIP(hipMemcpyAsync(faces.data(), ap.faces, (size_t)n * sizeof(AlignFace), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        const AlignFace &f = faces[i];
        mode[i] = f.mode;
        for (int k = 0; k < 6; ++k) M[6 * i + k] = f.M[k];
        roi[4 * i] = f.x0; roi[4 * i + 1] = f.y0; roi[4 * i + 2] = f.rw; roi[4 * i + 3] = f.rh;
        scale[2 * i] = f.scale_x; scale[2 * i + 1] = f.scale_y;
        area_fast[i] = f.area_fast;
    }
    return ctx_check_nms_flag(c);
}

int rfd_detect_select_align_batch(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_selection_config *sel_cfg, int is_enroll,
                                  const rfd_alignment_config *align_cfg, float *out_box, float *out_kps, int32_t *found,
                                  uint8_t *out_crops, int32_t *status)
{
    RFD_CHECK_ARG(c && out_crops && status, "null argument");
    const PreImage *frames;
    RFD_TRY(detect_select(c, imgs, n, sel_cfg, is_enroll, out_box, out_kps, found, &frames));
    SelView v;
    RFD_TRY(sel_own(ctx_face_stage(c), n, &v));
    return align_impl(c, frames, n, v, align_cfg, out_crops, status);
}

// ---- model inputs of the quality and ID stages (face_quality.rs:43-44,56-101, face_extraction.rs:38-77) ----
int rfd_face_tensors(rfd_ctx *c, const uint8_t *crops, int n, int crop_w, int crop_h, const rfd_face_tensor_config *cfgs, int k,
                     float *const *tensors)
{
    RFD_CHECK_ARG(c && crops, "null argument");
    RFD_TRY(check_face_tensor_args(cfgs, k, tensors, 1));
    RFD_PLAN(check_crop_size, crop_w, crop_h);
    RFD_TRY(ctx_check_batch(c, n, "batch"));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t crop = (size_t)crop_w * crop_h * 3;
    RFD_TRY(fs.face_in.reserve((size_t)n * crop));
    RFD_HIP(hipMemcpyAsync(fs.face_in.p, crops, (size_t)n * crop, hipMemcpyHostToDevice, s));
    const PlaneBytes planes = plane_bytes(cfgs, k);
    float *d_tensors[kMaxFaceTensors] = {};
    RFD_TRY(own_planes(fs, n, k, planes, d_tensors));
    FaceTensorParams tp;
    memset(&tp, 0, sizeof tp);
    tp.crops = (const uint8_t *)fs.face_in.p;
    tp.n = n; tp.crop_w = crop_w; tp.crop_h = crop_h; tp.k = k;
    for (int j = 0; j < k; ++j) fill_face_tensor_cfg(tp.cfg[j], cfgs[j], d_tensors[j], crop_w, crop_h);
    RFD_TRY(launch_face_tensors(tp, s));
    for (int j = 0; j < k; ++j) RFD_HIP(hipMemcpyAsync(tensors[j], d_tensors[j], n * planes.of[j], hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

int rfd_align_faces_tensors(rfd_ctx *c, const rfd_image *imgs, int n, const float *boxes, const float *kps, const int32_t *found,
                            const rfd_alignment_config *cfg, uint8_t *out_crops, int32_t *status,
                            const rfd_face_tensor_config *cfgs, int k, float *const *tensors)
{
    RFD_CHECK_ARG(c && boxes && kps && found && status, "null argument");
    RFD_TRY(check_face_tensor_args(cfgs, k, tensors, 0));
    rfd_alignment_config def;
    RFD_TRY(resolve_align_cfg(&cfg, &def));
    RFD_TRY(ctx_check_images(c, imgs, n));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const PreImage *frames;
    RFD_TRY(ctx_stage_frames(c, imgs, n, false, &frames));
    SelView v;
    RFD_TRY(sel_upload(c, n, boxes, kps, found, &v));
    return align_tensors_to_host(c, frames, n, cfg, out_crops, status, cfgs, k, tensors);
}

int rfd_detect_select_align_tensors_batch(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_selection_config *sel_cfg,
                                          int is_enroll, const rfd_alignment_config *align_cfg, float *out_box, float *out_kps,
                                          int32_t *found, uint8_t *out_crops, int32_t *status,
                                          const rfd_face_tensor_config *cfgs, int k, float *const *tensors)
{
    RFD_CHECK_ARG(c && status, "null argument");
    RFD_TRY(check_face_tensor_args(cfgs, k, tensors, 0));
    rfd_alignment_config def;
    RFD_TRY(resolve_align_cfg(&align_cfg, &def));
    const PreImage *frames;
    RFD_TRY(detect_select(c, imgs, n, sel_cfg, is_enroll, out_box, out_kps, found, &frames));
    return align_tensors_to_host(c, frames, n, align_cfg, out_crops, status, cfgs, k, tensors);
}

int rfd_detect_faces_device(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_selection_config *sel_cfg, int is_enroll,
                            const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k, rfd_faces *out,
                            int async)
{
    RFD_CHECK_ARG(c && out && out->box && out->kps && out->found && out->status, "null argument");
    RFD_TRY(check_face_tensor_args(cfgs, k, out->tensors, 0));
    RFD_TRY(ctx_check_images(c, imgs, n));
    rfd_dets dev;
    const PreImage *frames;
    RFD_TRY(ctx_detect_own_slabs(c, imgs, n, /*frames on device*/ true, &dev, &frames));
    const FrameSizes sz(imgs, n);
    RFD_TRY(select_enqueue(c, dev, sz.h.data(), sz.w.data(), n, sel_cfg, is_enroll, out->box, out->kps, out->found));
    rfd_alignment_config def;
    RFD_TRY(resolve_align_cfg(&align_cfg, &def));
    RFD_TRY(align_tensors_enqueue(c, frames, Faces{n, out->box, out->kps, out->found, nullptr, nullptr, 0}, *align_cfg, cfgs, k,
                                  FaceOut{out->crops, out->status, out->tensors}));
    return finish(c, async);
}

// ---- every detected face of a frame: the packed face list (rfd.h) ----
int rfd_align_detections(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_face_list_config *list_cfg,
                         const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k, int cap,
                         rfd_face_list *out)
{
    rfd_face_list_config ldef;
    rfd_alignment_config adef;
    RFD_TRY(check_face_list_call(c, imgs, n, &list_cfg, &ldef, &align_cfg, &adef, cfgs, k, cap, out));
    RFD_CHECK_ARG(dets && dets->boxes && dets->landmarks && dets->count, "detections are null");
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const PreImage *frames;
    RFD_TRY(ctx_stage_frames(c, imgs, n, false, &frames));
    rfd_dets dev = ctx_own_slabs(c);
    dev.total = nullptr; // the list does not read it
    RFD_TRY(ctx_copy_slabs(c, dev, *dets, n, hipMemcpyHostToDevice));
    return face_list_to_host(c, frames, n, dev, list_cfg, align_cfg, cfgs, k, cap, out);
}

int rfd_detect_align_all_batch(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_face_list_config *list_cfg,
                               const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k, int cap,
                               rfd_face_list *out)
{
    rfd_face_list_config ldef;
    rfd_alignment_config adef;
    RFD_TRY(check_face_list_call(c, imgs, n, &list_cfg, &ldef, &align_cfg, &adef, cfgs, k, cap, out));
    rfd_dets dev;
    const PreImage *frames; // they stay staged until the next call on this context
    RFD_TRY(ctx_detect_own_slabs(c, imgs, n, /*frames on device*/ false, &dev, &frames));
    return face_list_to_host(c, frames, n, dev, list_cfg, align_cfg, cfgs, k, cap, out);
}

int rfd_detect_all_faces_device(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_face_list_config *list_cfg,
                                const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k, int cap,
                                rfd_face_list *out, int async)
{
    rfd_face_list_config ldef;
    rfd_alignment_config adef;
    RFD_TRY(check_face_list_call(c, imgs, n, &list_cfg, &ldef, &align_cfg, &adef, cfgs, k, cap, out));
    rfd_dets dev;
    const PreImage *frames;
    RFD_TRY(ctx_detect_own_slabs(c, imgs, n, /*frames on device*/ true, &dev, &frames));
    RFD_TRY(face_list_enqueue(c, frames, n, dev, list_cfg, align_cfg, cfgs, k, cap, *out));
    return finish(c, async);
}

// The device-resident form of rfd_align_detections: the frames' descriptors, then the list over the caller's device slabs.
int rfd_align_detections_device(rfd_ctx *c, const rfd_image *imgs, int n, const rfd_dets *dets, const rfd_face_list_config *list_cfg,
                                const rfd_alignment_config *align_cfg, const rfd_face_tensor_config *cfgs, int k, int cap,
                                rfd_face_list *out, int async)
{
    rfd_face_list_config ldef;
    rfd_alignment_config adef;
    RFD_TRY(check_face_list_call(c, imgs, n, &list_cfg, &ldef, &align_cfg, &adef, cfgs, k, cap, out));
    RFD_CHECK_ARG(dets && dets->boxes && dets->landmarks && dets->count, "detections are null");
    RFD_HIP(hipSetDevice(ctx_device(c)));
    const PreImage *frames;
    RFD_TRY(ctx_stage_frames(c, imgs, n, true, &frames));
    RFD_TRY(face_list_enqueue(c, frames, n, *dets, list_cfg, align_cfg, cfgs, k, cap, *out));
    return finish(c, async);
}

// ---- after the two models: quality decision rule (face_quality.rs:159-168), embedding normalisation (utils.rs:148-154) ----
int rfd_quality_decide_device(rfd_ctx *c, const float *logits, int n, int classes, float threshold, float *score, int32_t *klass)
{
    RFD_TRY(check_quality_args(c, logits, n, classes, score, klass));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    return launch_quality_decide(logits, n, classes, threshold, score, klass, ctx_stream(c));
}

int rfd_quality_decide(rfd_ctx *c, const float *logits, int n, int classes, float threshold, float *score, int32_t *klass)
{
    RFD_TRY(check_quality_args(c, logits, n, classes, score, klass));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t in_bytes = (size_t)n * classes * sizeof(float);
    RFD_TRY(fs.face_io[0].reserve(in_bytes));
    RFD_TRY(fs.face_io[1].reserve((size_t)n * (sizeof(float) + sizeof(int32_t))));
    float *d_score = (float *)fs.face_io[1].p;
    int32_t *d_klass = (int32_t *)(d_score + n);
    RFD_HIP(hipMemcpyAsync(fs.face_io[0].p, logits, in_bytes, hipMemcpyHostToDevice, s));
    RFD_TRY(rfd_quality_decide_device(c, (const float *)fs.face_io[0].p, n, classes, threshold, d_score, d_klass));
    RFD_HIP(hipMemcpyAsync(score, d_score, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(klass, d_klass, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        if (klass[i] < 0) { // the reference panics here (partial_cmp(..).unwrap(), face_quality.rs:160)
            set_error("invalid argument: the logits of frame %d hold a NaN", i);
            return RFD_ERR_INVALID_ARG;
        }
    return RFD_OK;
}

int rfd_normalize_embeddings_device(rfd_ctx *c, const float *emb, int n, int dim, float *out)
{
    RFD_TRY(check_normalize_args(c, emb, n, dim, out));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    return launch_l2_normalize(emb, n, dim, out, ctx_stream(c));
}

int rfd_normalize_embeddings(rfd_ctx *c, const float *emb, int n, int dim, float *out)
{
    RFD_TRY(check_normalize_args(c, emb, n, dim, out));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t bytes = (size_t)n * dim * sizeof(float);
    RFD_TRY(fs.face_io[0].reserve(bytes));
    RFD_TRY(fs.face_io[1].reserve(bytes));
    RFD_HIP(hipMemcpyAsync(fs.face_io[0].p, emb, bytes, hipMemcpyHostToDevice, s));
    RFD_TRY(rfd_normalize_embeddings_device(c, (const float *)fs.face_io[0].p, n, dim, (float *)fs.face_io[1].p));
    RFD_HIP(hipMemcpyAsync(out, fs.face_io[1].p, bytes, hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}

// ---- liveness (face_antispoofing.rs): the inputs of the miniFAS models from the frame and the selected box, and the rule
//      on their outputs.  The models themselves are remote, like the quality and the ID model. ----
int rfd_liveness_tensors_device(rfd_ctx *c, const rfd_image *imgs, int n, const float *boxes, const int32_t *found,
                                const rfd_liveness_config *cfg, float *const *tensors, float *weights, int32_t *rois,
                                int32_t *status, int async)
{
    rfd_liveness_config def;
    RFD_TRY(check_liveness_args(c, imgs, n, boxes, found, &cfg, &def, tensors, weights, status));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    RFD_TRY(liveness_enqueue(c, imgs, n, true, boxes, found, cfg, tensors, weights, rois, status));
    return finish(c, async);
}

int rfd_liveness_tensors(rfd_ctx *c, const rfd_image *imgs, int n, const float *boxes, const int32_t *found,
                         const rfd_liveness_config *cfg, float *const *tensors, float *weights, int32_t *rois, int32_t *status)
{
    rfd_liveness_config def;
    RFD_TRY(check_liveness_args(c, imgs, n, boxes, found, &cfg, &def, tensors, weights, status));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const int k = cfg->k;
    const LiveTensorLayout l = live_tensor_layout(n, k);
    RFD_TRY(fs.live_io.reserve(l.words * 4));
    float *o = (float *)fs.live_io.p;
    float *d_box = o + l.box, *d_weights = o + l.weights;
    int32_t *d_found = (int32_t *)(o + l.found), *d_rois = (int32_t *)(o + l.rois), *d_status = (int32_t *)(o + l.status);
    const PlaneBytes planes = plane_bytes(*cfg);
    float *d_tensors[kMaxFaceTensors] = {};
    RFD_TRY(own_planes(fs, n, k, planes, d_tensors));
    RFD_HIP(hipMemcpyAsync(d_box, boxes, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_HIP(hipMemcpyAsync(d_found, found, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    RFD_TRY(liveness_enqueue(c, imgs, n, false, d_box, d_found, cfg, d_tensors, d_weights, d_rois, d_status));
    for (int j = 0; j < k; ++j) RFD_HIP(hipMemcpyAsync(tensors[j], d_tensors[j], n * planes.of[j], hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(weights, d_weights, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, s));
    if (rois) RFD_HIP(hipMemcpyAsync(rois, d_rois, (size_t)n * k * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(status, d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return finish(c);
}

int rfd_liveness_decide_device(rfd_ctx *c, const float *const *logits, int k, int n, int classes, const float *weights,
                               float threshold, float *score, int32_t *live)
{
    RFD_TRY(check_liveness_decide_args(c, logits, k, n, classes, weights, score, live));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    if (k > kLiveDecideChunk) RFD_TRY(fs.live_acc.reserve((size_t)n * 2 * sizeof(float)));
    for (int j0 = 0; j0 < k; j0 += kLiveDecideChunk) {
        LiveLogits l;
        memset(&l, 0, sizeof l);
        const int kc = std::min(kLiveDecideChunk, k - j0);
        for (int q = 0; q < kc; ++q) l.p[q] = logits[j0 + q];
        RFD_TRY(launch_liveness_decide(l, kc, k, j0, n, classes, weights, threshold, (float *)fs.live_acc.p, score, live, ctx_stream(c)));
    }
    return RFD_OK;
}

int rfd_liveness_decide(rfd_ctx *c, const float *const *logits, int k, int n, int classes, const float *weights, float threshold,
                        float *score, int32_t *live)
{
    RFD_TRY(check_liveness_decide_args(c, logits, k, n, classes, weights, score, live));
    RFD_HIP(hipSetDevice(ctx_device(c)));
    FaceStage &fs = ctx_face_stage(c);
    const hipStream_t s = ctx_stream(c);
    const size_t one = (size_t)n * classes;
    const LiveDecideLayout l = live_decide_layout(n, k, classes);
    RFD_TRY(fs.live_io.reserve(l.words * 4));
    float *o = (float *)fs.live_io.p;
    float *d_logits = o + l.logits, *d_weights = o + l.weights, *d_score = o + l.score;
    int32_t *d_live = (int32_t *)(o + l.live);
    std::vector<const float *> ptrs(k);
    for (int j = 0; j < k; ++j) {
        ptrs[j] = d_logits + (size_t)j * one;
        RFD_HIP(hipMemcpyAsync(d_logits + (size_t)j * one, logits[j], one * sizeof(float), hipMemcpyHostToDevice, s));
    }
    RFD_HIP(hipMemcpyAsync(d_weights, weights, (size_t)n * k * sizeof(float), hipMemcpyHostToDevice, s));
    RFD_TRY(rfd_liveness_decide_device(c, ptrs.data(), k, n, classes, d_weights, threshold, d_score, d_live));
    RFD_HIP(hipMemcpyAsync(score, d_score, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipMemcpyAsync(live, d_live, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RFD_HIP(hipStreamSynchronize(s));
    return RFD_OK;
}
