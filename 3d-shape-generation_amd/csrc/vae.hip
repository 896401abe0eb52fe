// a12: VAE3DLarge.encode / decode (reference networks.py:2299-2310, 2327-2339; nets :2225-2264, ResidualBlock3D
// :471-504) as single enqueues behind a handle.
//
// Host-side sequencing only: every launch goes through the layer-level entry points of this library (direct first /
// last layers, LDS-halo k3 convolution, implicit-GEMM convolution with the ConvTranspose3d parity classes in one
// launch and split-K for the small-grid layers, fp16 GEMMs for the Linear layers).  Activations NDHWC fp16, eval-mode
// BatchNorm3d folded into the weights by the host packer.
#include <new>
#include <utility>
#include "common.h"

struct pcd_vae {
    pcd_vae_desc_t d;
    // Fragment-order copies of the k3 layers' weights (pcd_conv3d_pack_wfrag), made at create and keyed by the layer of `d` they belong to;
    // a conv2 with a fused projection shortcut carries the shortcut's columns as "tap 27".  wf == null: that layer keeps the LDS-ring kernel.
    struct Frag { const pcd_vae_conv_t* L; void* wf; };
    Frag frag[11] = {};
    void* wf_last = nullptr;            // decoder.12's weights as MFMA A operands (pcd_conv3d_last_pack)

    const void* wfrag(const pcd_vae_conv_t& L) const {
        for (const Frag& f : frag) if (f.L == &L) return f.wf;
        return nullptr;
    }
};

namespace pcd {

// three rotating activation buffers (the largest activation is 32^3 x 64 channels), the split-K scratch of the
// convolution launches, and the small GEMM operands
struct VaeWs { size_t a, b, c, scratch, scratch_bytes, small, total; };
static constexpr size_t kConvScratchPerSample = (size_t)8 << 20;     // >= the split-K slabs of any layer (checked per launch)
static VaeWs vae_carve(int batch) {
    VaeWs w{};
    const size_t act = align_up((size_t)batch * 32768 * 64 * 2);
    size_t o = 0;
    w.a = o; o += act;
    w.b = o; o += act;
    w.c = o; o += act;
    w.scratch = o;
    w.scratch_bytes = align_up(kConvScratchPerSample * (size_t)(batch < 4 ? 4 : batch));
    o += w.scratch_bytes;
    w.small = o; o += align_up((size_t)batch * 1024 * 4);
    w.total = o;
    return w;
}

// pcd_vae_config, decoded: the LDS-halo / weights-in-registers forms in use (the table of codes is in include/pcd_hip.h).  TEST / BENCHMARK ONLY, process-global.
enum { kCfgConvT = 2, kCfgK4S2 = 4, kCfgWreg = 8 };
static int g_vae_forms = kCfgConvT | kCfgK4S2 | kCfgWreg;

struct ConvGeom { int din, stride; const int* taps; int dout; };    // input grid, stride, tap table and output grid of a layer (cubes)

struct Runner {
    const pcd_vae& h;
    const pcd_vae_desc_t& d;
    int batch;
    char* scratch;
    size_t scratch_bytes;
    hipStream_t s;
    void *x, *hb, *r;                 // x: the current activation (a layer or block leaves its output there, whichever buffer that is); hb, r: the other two

    ConvGeom k3(int dim) const { return {dim, 1, d.taps3, dim}; }           // k3 s1 p1
    ConvGeom k1(int dim) const { return {dim, 1, d.taps1, dim}; }           // 1x1x1
    ConvGeom down(int din) const { return {din, 2, d.taps4s2, din / 2}; }   // k4 s2 p1
    ConvGeom flat(int din) const { return {din, 1, d.taps4p0, 1}; }         // k4 p0 over the whole grid

    int launch(const pcd_conv3d_desc_t* descs, int n) const {
        size_t need = pcd_conv3d_workspace_bytes(descs, n);
        if (need > scratch_bytes) need = 0;                           // too small: the launch simply runs unsplit
        return pcd_conv3d_f16_multi(descs, n, need ? scratch : nullptr, need, s);
    }
    pcd_conv3d_desc_t desc(const pcd_vae_conv_t& L, int ntaps, const void* in, ConvGeom g, void* out, int relu, const void* resid, const void* in2, int cin2) const {
        pcd_conv3d_desc_t c{};
        c.in = in; c.batch = batch; c.in_d = c.in_h = c.in_w = g.din; c.cin = L.cin;
        c.rows_d = c.rows_h = c.rows_w = g.dout; c.stride = g.stride;
        c.taps = g.taps; c.ntaps = ntaps; c.kpad = L.kpad;
        c.w = L.w; c.bias = L.b; c.resid = resid; c.relu = relu;
        c.out = out; c.cout = L.cout;
        c.out_d = c.out_h = c.out_w = g.dout; c.out_scale = 1;
        c.zero_page = d.zero_page;
        c.in2 = in2; c.cin2 = in2 ? cin2 : 0;
        return c;
    }
    // Conv3d(k, stride, pad) [+ residual | + a second source behind the taps] [+ ReLU]
    int conv(const pcd_vae_conv_t& L, const void* in, ConvGeom g, void* out, int relu = 1, const void* resid = nullptr, const void* in2 = nullptr,
             int cin2 = 0) const {
        const pcd_conv3d_desc_t c = desc(L, L.k * L.k * L.k, in, g, out, relu, resid, in2, cin2);
        // k3 layers with a fragment-order copy: weights in registers, 256-row workgroups, no barrier in the tap loop
        const void* wfrag = h.wfrag(L);
        if (wfrag != nullptr && (g_vae_forms & kCfgWreg) && pcd_conv3d_k3s1_wreg_supported(&c)) return pcd_conv3d_k3s1_wreg_f16(&c, wfrag, s);
        if (L.k == 3 && g.stride == 1 && pcd_conv3d_k3s1_supported(&c)) return pcd_conv3d_k3s1_f16(&c, s);   // LDS-resident halo
        // encoder.3 (k4 s2, 64 -> 64, 32^3 -> 16^3): the eight input-parity classes from LDS-resident sub-grid halos
        if ((g_vae_forms & kCfgK4S2) && L.k == 4 && g.stride == 2 && resid == nullptr && in2 == nullptr && g.dout * 2 == g.din &&
            pcd_conv3d_k4s2_halo_supported(batch, g.din, g.din, g.din, L.cin, L.cout, L.kpad))
            return pcd_conv3d_k4s2_halo_f16(in, batch, g.din, g.din, g.din, L.cin, L.w, L.kpad, L.b, relu, L.cout, out, s);
        return launch(&c, 1);
    }
    // one layer from x into hb, which becomes x
    int step(const pcd_vae_conv_t& L, ConvGeom g) { const int rc = conv(L, x, g, hb); std::swap(x, hb); return rc; }
    int up(const pcd_vae_convT_t& T, int din) { const int rc = convT(T, x, din, hb); std::swap(x, hb); return rc; }
    // ResidualBlock3D: relu(bn2(conv2(relu(bn1(conv1 x)))) + (downsample(x) | x))
    int res(const pcd_vae_res_t& R, int dim) {
        int rc = conv(R.c1, x, k3(dim), hb);
        if (rc) return rc;
        const void* resid = x;
        if (R.has_ds && R.fused_ds) {
            // projection shortcut inside conv2's launch: its weights are K columns behind the 27 taps, x the second source.  NOT in
            // place: rows of x (ds.cin channels) and rows of the output (c2.cout channels) have different strides
            rc = conv(R.c2, hb, k3(dim), r, 1, nullptr, x, R.ds.cin);
            std::swap(x, r);
            return rc;
        }
        if (R.has_ds) {
            // 1x1x1 shortcut + BN: a pointwise layer over the NDHWC rows (weights in LDS) where the shape has one
            if (pcd_conv1x1_supported(R.ds.cin, R.ds.cout))
                rc = pcd_conv1x1_f16(x, (int64_t)batch * dim * dim * dim, R.ds.cin, R.ds.w, R.ds.kpad, R.ds.b, 0, R.ds.cout, r, s);
            else
                rc = conv(R.ds, x, k1(dim), r, 0);
            if (rc) return rc;
            resid = r;
        }
        return conv(R.c2, hb, k3(dim), x, 1, resid);                  // in place: conv2 reads hb and the residual row it overwrites
    }
    // ConvTranspose3d(k4, s2, p1) + ReLU: the 8 output-parity classes (2x2x2 taps each) in one launch
    int convT(const pcd_vae_convT_t& T, const void* in, int din, void* out) const {
        // decoder.6 (128 -> 64, 16^3 -> 32^3): all eight classes from one LDS-resident input halo
        if ((g_vae_forms & kCfgConvT) && pcd_convt3d_k4s2_halo_supported(batch, din, din, din, T.cin, T.cout))
            return pcd_convt3d_k4s2_halo_f16(in, batch, din, din, din, T.cin, T.w, T.b, T.cout, out, s);
        pcd_conv3d_desc_t c[8];
        for (int k = 0; k < 8; ++k) {              // a stride-1 layer of 2 x 2 x 2 taps on the input grid, written to every other voxel of the output grid
            pcd_vae_conv_t L{};
            L.w = T.w[k]; L.b = T.b; L.kpad = 8 * T.cin; L.cin = T.cin; L.cout = T.cout; L.k = 2;
            c[k] = desc(L, 8, in, {din, 1, T.taps[k], din}, out, 1, nullptr, nullptr, 0);
            c[k].out_d = c[k].out_h = c[k].out_w = 2 * din; c[k].out_scale = 2;
            c[k].out_off_z = (k >> 2) & 1; c[k].out_off_y = (k >> 1) & 1; c[k].out_off_x = k & 1;
        }
        return launch(c, 8);
    }
};

static bool conv_ok(const pcd_vae_conv_t& L) { return L.w && L.b && L.cin > 0 && L.cout > 0 && L.kpad > 0 && L.k > 0; }
static bool res_ok(const pcd_vae_res_t& R) {
    if (!conv_ok(R.c1) || !conv_ok(R.c2)) return false;
    if (R.has_ds && R.fused_ds)
        return R.ds.cin >= 32 && R.ds.cout == R.c2.cout && R.c2.kpad >= 27 * R.c2.cin + R.ds.cin &&
               (R.ds.cin == 32 || R.c2.kpad == 27 * R.c2.cin + R.ds.cin);
    return !R.has_ds || conv_ok(R.ds);
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_vae_config(int v) {
    PCD_CHECK_ARG(v >= 0 && v <= 15);
    g_vae_forms = v == 1 ? 14 : (v & 14);
    return PCD_OK;
}

extern "C" int pcd_vae_create(const pcd_vae_desc_t* desc, pcd_vae_t** out) {
    PCD_CHECK_ARG(desc != nullptr && out != nullptr);
    PCD_CHECK_ARG(desc->latent_dim > 0 && desc->latent_dim % 64 == 0);
    PCD_CHECK_ARG(desc->enc0_w && desc->enc0_b && desc->fc_w && desc->fc_b && desc->din_w && desc->din_b && desc->last_w);
    PCD_CHECK_ARG(desc->taps3 && desc->taps4s2 && desc->taps4p0 && desc->taps1 && desc->zero_page);
    for (int i = 0; i < 4; ++i) PCD_CHECK_ARG(res_ok(desc->enc_res[i]) && res_ok(desc->dec_res[i]));
    for (int i = 0; i < 3; ++i) {
        PCD_CHECK_ARG(conv_ok(desc->enc_down[i]) && desc->dec_up[i].b && desc->dec_up[i].cin > 0 && desc->dec_up[i].cout > 0);
        for (int k = 0; k < 8; ++k) PCD_CHECK_ARG(desc->dec_up[i].w[k] && desc->dec_up[i].taps[k]);
    }
    PCD_CHECK_ARG(conv_ok(desc->enc_last) && conv_ok(desc->dec_conv9));
    // the channel plan of networks.py:2225-2264
    PCD_CHECK_ARG(desc->enc_res[0].c1.cin == 32 && desc->enc_res[3].c2.cout == 512 && desc->enc_last.cout == 512);
    PCD_CHECK_ARG(desc->dec_up[0].cin == 512 && desc->dec_conv9.cin == 64 && desc->dec_conv9.cout == 32);
    pcd_vae* h = new (std::nothrow) pcd_vae;
    PCD_CHECK_ARG(h != nullptr);
    h->d = *desc;
    // fragment-order weight copies (one-time device work on the null stream, finished before the handle is returned); a failed copy only
    // means that layer keeps the LDS-ring kernel
    const pcd_vae_conv_t* const layers[11] = {&h->d.enc_res[1].c1, &h->d.dec_res[2].c1, &h->d.dec_res[2].c2, &h->d.enc_res[0].c2, &h->d.enc_res[0].c1, &h->d.dec_res[3].c1,
                                              &h->d.dec_res[3].c2, &h->d.dec_conv9,     &h->d.enc_res[1].c2, &h->d.dec_res[1].c1, &h->d.dec_res[1].c2};
    for (int i = 0; i < 11; ++i) {
        const pcd_vae_conv_t& L = *layers[i];
        const size_t bytes = L.k == 3 && L.kpad >= 27 * L.cin ? pcd_conv3d_wfrag_bytes(L.cin, L.cout) : 0;
        // a fused projection shortcut's columns sit behind the 27 taps: up to kpad - 27 cin of them (the packer pads K to a multiple of 64 with zeros)
        const int extra = L.kpad - 27 * L.cin, cin2 = L.cin >= 64 ? (extra >= 64 ? 64 : (extra >= 32 ? 32 : 0)) : 0;
        h->frag[i] = {&L, pcd_packed_copy(L.w, bytes, [&](void* buf) { return pcd_conv3d_pack_wfrag(L.w, L.kpad, L.cin, L.cout, cin2, buf, nullptr); })};
    }
    // decoder.12's weights as MFMA A operands (27 KB); a failure leaves the VALU form
    h->wf_last = pcd_packed_copy(desc->last_w, pcd_conv3d_last_packed_bytes(), [&](void* buf) { return pcd_conv3d_last_pack(desc->last_w, buf, nullptr); });
    *out = h;
    return PCD_OK;
}

extern "C" void pcd_vae_destroy(pcd_vae_t* h) {
    if (h == nullptr) return;
    if (h->wf_last) (void)hipFree(h->wf_last);
    for (const pcd_vae::Frag& f : h->frag)
        if (f.wf != nullptr) (void)hipFree(f.wf);
    delete h;
}

extern "C" size_t pcd_vae_workspace_bytes(int batch) {
    if (batch <= 0) return 0;
    return vae_carve(batch).total;
}

#define VAE_PROLOGUE()                                                                        \
    const VaeWs w = vae_carve(batch);                                                         \
    if (workspace_bytes < w.total) {                                                          \
        set_error("%s: workspace %zu < required %zu", __func__, workspace_bytes, w.total);    \
        return PCD_ERR_WORKSPACE;                                                             \
    }                                                                                         \
    char* ws = (char*)workspace;                                                              \
    const pcd_vae_desc_t& d = h->d;                                                           \
    hipStream_t s = (hipStream_t)stream;                                                      \
    Runner R{*h, d, batch, ws + w.scratch, w.scratch_bytes, s, ws + w.a, ws + w.b, ws + w.c};     \
    int rc

extern "C" int pcd_vae_encode(pcd_vae_t* h, const float* vox, int batch, float* mu_logvar, void* workspace,
                              size_t workspace_bytes, void* stream) {
    PCD_CHECK_ARG(h && vox && mu_logvar && workspace && batch > 0);
    VAE_PROLOGUE();
    // encoder.0/1: Conv3d(1, 32, k3, p1) + ReLU straight from the fp32 occupancy grid
    PCD_RUN(pcd_conv3d_first(vox, batch, 32, 32, 32, 1, d.enc0_w, d.enc0_b, 32, R.x, s));
    PCD_RUN(R.res(d.enc_res[0], 32));                       // encoder.2   32 -> 64 @ 32^3
    PCD_RUN(R.step(d.enc_down[0], R.down(32)));             // encoder.3/4 k4 s2 -> 16^3
    PCD_RUN(R.res(d.enc_res[1], 16));                       // encoder.5   64 -> 128
    PCD_RUN(R.step(d.enc_down[1], R.down(16)));             // encoder.6/7 -> 8^3
    PCD_RUN(R.res(d.enc_res[2], 8));                        // encoder.8   128 -> 256
    PCD_RUN(R.step(d.enc_down[2], R.down(8)));              // encoder.9/10 -> 4^3
    PCD_RUN(R.res(d.enc_res[3], 4));                        // encoder.11  256 -> 512
    void* const B = R.x; void* const A = R.hb;                                   // below: B = encoder.11's output, A = scratch
    // encoder.12/13: k4 p0 on a 4^3 grid = one row of 32768 inputs per sample -> (B, 512).  With <= 256 samples that is the
    // weight-streaming GEMM of the latent denoiser (33.5 MB of weights against B rows), not a 128-row convolution tile
    const int k_last = d.enc_last.cin * 64;
    const size_t slab_bytes = (size_t)pcd_skinny_slabs(k_last, d.enc_last.cout) * batch * d.enc_last.cout * sizeof(float);
    if (batch <= 256 && d.enc_last.kpad == k_last && slab_bytes <= w.scratch_bytes) {
        float* slabs = (float*)(ws + w.scratch);
        PCD_RUN(pcd_skinny_gemm_f16(B, k_last, nullptr, 0, d.enc_last.w, d.enc_last.kpad, batch, d.enc_last.cout, slabs, s));
        PCD_RUN(pcd_skinny_finish(slabs, pcd_skinny_slabs(k_last, d.enc_last.cout), batch, d.enc_last.cout, d.enc_last.b, nullptr,
                              1, 0, nullptr, nullptr, A, nullptr, s));
    } else {
        PCD_RUN(R.conv(d.enc_last, B, R.flat(4), A));
    }
    // [fc_mu ; fc_logvar]: 512 -> 2 * latent, fp32 out
    const int c_fc = 2 * d.latent_dim, s_fc = pcd_skinny_slabs(512, c_fc);
    if (batch <= 256 && (size_t)s_fc * batch * c_fc * sizeof(float) <= w.scratch_bytes) {
        float* slabs = (float*)(ws + w.scratch);
        PCD_RUN(pcd_skinny_gemm_f16(A, 512, nullptr, 0, d.fc_w, 512, batch, c_fc, slabs, s));
        PCD_RUN(pcd_skinny_finish(slabs, s_fc, batch, c_fc, d.fc_b, nullptr, 2, 0, nullptr, nullptr, nullptr, mu_logvar, s));
    } else {
        pcd_gemm_desc_t g{};
        g.a1 = A; g.k1 = 512; g.lda1 = 512; g.w = d.fc_w; g.ldw = 512; g.bias = d.fc_b; g.relu = 0; g.m = batch;
        g.c = c_fc;
        PCD_RUN(pcd_gemm_f16_out32(&g, mu_logvar, c_fc, s));
    }
    return PCD_OK;
}

extern "C" int pcd_vae_decode(pcd_vae_t* h, const float* z, int batch, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    PCD_CHECK_ARG(h && z && out && workspace && batch > 0);
    VAE_PROLOGUE();
    void* z16 = ws + w.small;
    PCD_RUN(pcd_f32_to_f16(z, z16, (int64_t)batch * d.latent_dim, s));
    pcd_gemm_desc_t g{};                                                         // decoder_input, columns already in NDHWC order
    g.a1 = z16; g.k1 = d.latent_dim; g.lda1 = d.latent_dim; g.w = d.din_w; g.ldw = d.latent_dim; g.bias = d.din_b;
    g.relu = 0; g.m = batch; g.c = 512 * 64;
    PCD_RUN(pcd_gemm_f16(&g, R.x, 512 * 64, s));                                     // (B, 4,4,4, 512)
    PCD_RUN(R.up(d.dec_up[0], 4));                          // decoder.0/1  512 -> 256 @ 8^3
    PCD_RUN(R.res(d.dec_res[0], 8));                        // decoder.2
    PCD_RUN(R.up(d.dec_up[1], 8));                          // decoder.3/4  256 -> 128 @ 16^3
    PCD_RUN(R.res(d.dec_res[1], 16));                       // decoder.5
    PCD_RUN(R.up(d.dec_up[2], 16));                         // decoder.6/7  128 -> 64 @ 32^3
    PCD_RUN(R.res(d.dec_res[2], 32));                       // decoder.8
    PCD_RUN(R.step(d.dec_conv9, R.k3(32)));                 // decoder.9/10  64 -> 32
    PCD_RUN(R.res(d.dec_res[3], 32));                       // decoder.11
    PCD_RUN(pcd_conv3d_last_sigmoid_packed(R.x, batch, 32, 32, 32, 32, d.last_w, h->wf_last, d.last_b, out, s));   // decoder.12/13
    return PCD_OK;
}
#undef VAE_PROLOGUE
