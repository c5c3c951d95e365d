// shapegan_amd/csrc/conv_common.h — geometry helpers shared by the k4/s2/p1 convolution kernels.
#pragma once
#include "common.h"

namespace sg {

// n / d for n < 2^31 with precomputed magic (round-up method)
struct FastDiv {
    uint32_t m, s, d;
    FastDiv() : m(0), s(0), d(1) {}
    explicit FastDiv(uint32_t dd) : d(dd) {
        s = 0;
        while ((1u << s) < dd) ++s;
        m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << s) - dd)) / dd + 1);
    }
    __device__ __forceinline__ uint32_t div(uint32_t n) const { return (__umulhi(n, m) + n) >> s; }
    __device__ __forceinline__ void divmod(uint32_t n, uint32_t& q, uint32_t& r) const {
        q = div(n);
        r = n - q * d;
    }
};

struct ConvGeom {
    int ID, IH, IW;   // spatial size of the stride-1 side (x of the conv)
    int OD, OH, OW;   // spatial size of the stride-2 side (y of the conv) = I/2
    int Cx, Cy;       // channels physically present in x / y tensors (batch strides)
    FastDiv dOW, dOH, dOD;
    long I3() const { return (long)ID * IH * IW; }
    long O3() const { return (long)OD * OH * OW; }
};

// decode a flat (n,od,oh,ow) position of the O grid
__device__ __forceinline__ void decode_pos(const ConvGeom& g, uint32_t j, int& n, int& od, int& oh, int& ow) {
    uint32_t t1, t2, t3, a, b, c;
    g.dOW.divmod(j, t1, a);
    g.dOH.divmod(t1, t2, b);
    g.dOD.divmod(t2, t3, c);
    ow = (int)a;
    oh = (int)b;
    od = (int)c;
    n = (int)t3;
}

static inline int make_geom(ConvGeom& g, int ID, int IH, int IW, int Cx, int Cy) {
    if (ID < 2 || IH < 2 || IW < 2 || (ID & 1) || (IH & 1) || (IW & 1)) return -1;
    g.ID = ID;
    g.IH = IH;
    g.IW = IW;
    g.OD = ID / 2;
    g.OH = IH / 2;
    g.OW = IW / 2;
    g.Cx = Cx;
    g.Cy = Cy;
    g.dOW = FastDiv(g.OW);
    g.dOH = FastDiv(g.OH);
    g.dOD = FastDiv(g.OD);
    return 0;
}


// ================================================================================================================
// Host-side plans.  Every k4/s2/p1 call is planned ONCE by a pure host function (no pointers, no streams): whether a kernel family
// serves it, which kernel, its grid / block / LDS bytes, the image it reads from the workspace and the workspace bytes it needs.
// The pack and launch functions below take a plan plus the real pointers; the size queries, sg_conv3d_k4s2p1_pack_images,
// sg_conv3d_k4s2p1_image_layout and the eligibility queries of the C ABI read the same plans (conv3d.hip).
// `workspace_bytes` of a plan function is what the call may use: 0 when it has no workspace.

struct KernelPlan {
    bool served;              // false: this kernel family does not take the call (the caller goes on to the next one)
    dim3 grid;
    unsigned block;
    size_t lds;               // dynamic LDS bytes
    size_t workspace_need;    // bytes of workspace the call needs to be served
};
template <class T>
static inline T* workspace_at(void* workspace, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(workspace) + offset); }

// An image a kernel reads from the workspace: the packed form, its row tiles, and where it starts.
struct ImageJob {
    int kind;        // weight images: 0 / 2 forward image mode 0 / 1, 1 / 3 input-gradient image mode 0 / 1 (pack_images_kernel);
                     // the weight gradient's dy image: 0 = 8-divisible grids, 1 = 4^3
    int nt;          // forward image: 32-row tiles; input-gradient image: MT; dy image: mt_total
    size_t offset;   // bytes from the start of the workspace
};

// Packing jobs of the LDS-halo kernels' weight images, taken from the plans of up to 8 forthcoming calls and launched together
// (conv3d_halo.hip: pack_images_kernel, sg_conv3d_k4s2p1_pack_images)
struct PackJob {
    const float* w;
    float4* wp;
    int kind, Cout, Cin_total, Cin, nt;     // ImageJob kind and nt
};
struct PackJobs {
    PackJob job[8];
    int n = 0;
    int add(const ImageJob& image, const float* w, void* workspace, int Cout, int Cin_total, int Cin) {
        if (n >= 8) return 0;
        job[n++] = PackJob{w, workspace_at<float4>(workspace, image.offset), image.kind, Cout, Cin_total, Cin, image.nt};
        return 1;
    }
};
int halo_pack_jobs_launch(const PackJobs& jobs, hipStream_t stream);

// ---- conv3d_halo.hip: the LDS-halo kernels ----------------------------------------------------------------------------------------
// The forms tests and tuning select through sg_conv3d_k4s2p1_fwd_impl / _dgrad_impl, decoded once from the ABI's integers
// (include/shapegan_hip.h states the bit values).  All fields zero = the dispatch rule of the product calls.
struct HaloFwdForm {
    bool forced;         // impl 1: no dispatch thresholds, no channel split
    int variant;         // debug bits 4-5: 0 the default, 1 = 4 waves x 2 row tiles, 2 = 8 waves x 1, 3 = 64-row tiles
    bool keep_lds;       // debug bit 6: do not raise the LDS request to cap the CU at two workgroups
    bool keep_rows128;   // debug bit 7: 128-row tiles at any grid size
    bool dskip;          // debug bit 8: the depth-skip form of the 4^3 kernel (refused on other grids)
};
HaloFwdForm halo_fwd_form_decode(int debug);      // (of a forced call)
struct HaloDgradForm {
    bool forced;         // impl bit 0
    bool one_parity;     // impl bit 1 (impl 3): one output parity per workgroup
    int ppw;             // impl bits 2-5 (impl 1 + 4 ppw): 2, 4 or 8 parities per workgroup
    bool rows64_dskip;   // impl bit 6: 64-row workgroups at any size, in the depth-skip form (4^3 grids only)
    bool depth_walk;     // impl bit 7: 64-row workgroups at any size, in the depth-walk form (dy grids of depth 8 only)
};
bool halo_dgrad_form_decode(int impl, HaloDgradForm* form);      // false: bits the ABI does not define

size_t halo_fwd_workspace_bytes(int Cin, int Cout);       // the forward weight image
constexpr int kHaloFwd4MaxSplit = 8;                      // 4^3 forward: at most this many channel-split partials behind the image
enum class HaloFwdKernel { halo4, halo4_dskip, rows128_w8, rows128_w4, rows64 };
struct HaloFwdPlan : KernelPlan {
    HaloFwdKernel kernel;
    ImageJob image;
    int nth, ntw;            // position tiles per H / W
    int csplit;               // 4^3 at small batches: the input channels split over this many workgroups (grid z), whose partial
    size_t partial_offset;    // sums lie at this byte offset and are finished by the caller (splitk_finalize_kernel, conv3d.hip)
};
HaloFwdPlan halo_fwd_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, HaloFwdForm form = HaloFwdForm());
void halo_fwd_pack(const HaloFwdPlan& p, const float* w, int Cin, int Cin_total, int Cout, void* workspace, hipStream_t stream);
void halo_fwd_launch(const HaloFwdPlan& p, const float* x, const float* bias, float* y, int batch, int Cin, int Cout, const ConvGeom& g,
                     int act, float slope, void* workspace, hipStream_t stream);

size_t halo_dgrad_workspace_bytes(int Cin, int Cout);     // the input-gradient weight image
// (_4: the 4^3 box of two samples; rows64_dwalk: the depth-walk form for dy grids of depth 8; SG_DGRAD_FORM_* of the ABI = 1 + these values)
enum class HaloDgradKernel { dskip4, rows32_4, rows64_4, rows32, rows64, rows64_dwalk };
struct HaloDgradPlan : KernelPlan {
    HaloDgradKernel kernel;
    ImageJob image;
    int mtiles, ppw;          // row tiles of 64 per parity; output parities per workgroup
    int ntd, nth, ntw;        // position tiles per D / H / W
};
HaloDgradPlan halo_dgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, HaloDgradForm form = HaloDgradForm());
void halo_dgrad_pack(const HaloDgradPlan& p, const float* w, int Cin, int Cin_total, int Cout, void* workspace, hipStream_t stream);
void halo_dgrad_launch(const HaloDgradPlan& p, const float* dy, const float* bias, float* dx, int batch, int Cin, int Cout,
                       const ConvGeom& g, int act, float slope, void* workspace, hipStream_t stream);

enum class HaloWgradKernel { halo4, rows64, rows128_skip_h, rows128 };
struct HaloWgradPlan : KernelPlan {      // (workspace_need: set for every shape the kernels exist for, served or not)
    HaloWgradKernel kernel;
    ImageJob dy_image;        // packed dy, [mt_total][nslice][8][64] float4 at the start of the workspace
    bool producer_image;      // dy's producer may write that image itself (sg_conv3d_k4s2p1_wgrad_dy_image)
    int nslice, nsplit, per_split, mtiles;      // nsplit = grid z
    size_t partial_offset;    // the nsplit > 1 partials behind the image
};
HaloWgradPlan halo_wgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, bool forced);
void halo_wgrad_pack(const HaloWgradPlan& p, const float* dy, int Cout, const ConvGeom& g, void* workspace, hipStream_t stream);
void halo_wgrad_launch(const HaloWgradPlan& p, const float* x, float* dw, int Cin, int Cin_total, int Cout, const ConvGeom& g,
                       void* workspace, hipStream_t stream);
int halo_act_bwd_pack8_launch(const float* y, const float* dy, float* dz, float* rowsum, void* ap, long rows, int C, long nslice,
                              int act, float slope, hipStream_t stream);

// ---- conv3d_edge.hip: layers with one channel on the voxel-grid side (Cin == 1, Cout <= 64) -------------------------------------------
// The forward and the plane-walk kernels read the grid in place (workspace_need 0).
enum class EdgeFwdKernel { lds_staged, gather };
struct EdgeFwdPlan : KernelPlan {
    EdgeFwdKernel kernel;
    int nt, actk;                 // the instantiation: row tiles of 32 channels; epilogue 0 none, 1 LeakyReLU as max(t, slope t), 2 generic
    int bh, units_per_wg;         // lds_staged: rows of a block, units per workgroup
};
EdgeFwdPlan edge_fwd_plan(int batch, int Cin, int Cout, const ConvGeom& g, int act, float slope);
void edge_fwd_launch(const EdgeFwdPlan& p, const float* x, const float* w, const float* bias, float* y, int batch, int Cin_total,
                     int Cout, const ConvGeom& g, int act, float slope, hipStream_t stream);

struct EdgeWgradPlan : KernelPlan {      // conv_wgrad_c1_kernel<nt, fuse>; its partial tiles are summed by wgrad_c1_finalize_kernel
    int nt, fuse;                 // fuse: 0, or the activation whose backward is formed in the kernel (SG_ACT_LEAKY / SG_ACT_RELU)
};
// fuse_act != 0: the weight + bias gradient straight from the gradient w.r.t. the activated output (sg_conv3d_k4s2p1_wgrad_act)
EdgeWgradPlan edge_wgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, int fuse_act);
void edge_wgrad_launch(const EdgeWgradPlan& p, const float* dy, const float* y, const float* x, float* dw, float* db, int batch,
                       int Cin_total, int Cout, const ConvGeom& g, float slope, void* workspace, hipStream_t stream);

enum class EdgeDgradKernel { walk_one_pair, walk_all_taps, plane_fused, tap_planes };
struct EdgeDgradPlan : KernelPlan {      // (workspace_need: the [batch][64][O3] tap planes that col2im_c1_kernel gathers)
    EdgeDgradKernel kernel;
    int splits;                  // plane walks: plane ranges per sample
};
// the plane-walk kernels alone, in a `form` of sg_convT3d_k4s2p1_to1_pre_impl (0: their dispatch rule)
EdgeDgradPlan edge_dgrad_walk_plan(int form, int batch, int Cin, int Cout, const ConvGeom& g);
EdgeDgradPlan edge_dgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes);
// in_scale != NULL (plane walks only): the input transform act_in(dy * in_scale[c] + in_shift[c]) folded into the loads
void edge_dgrad_launch(const EdgeDgradPlan& p, const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin_total,
                       int Cout, const ConvGeom& g, int act, float slope, void* workspace, hipStream_t stream,
                       const float* in_scale = nullptr, const float* in_shift = nullptr, int in_act = 0, float in_slope = 0.f,
                       int samples_per_group = 0, long out_group_stride = 0);

}  // namespace sg
