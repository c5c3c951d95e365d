// shapegan_amd/csrc_cpu/shapegan_cpu.cpp — libshapegan_cpu.so: the plain-C++ twin of the C ABI (include/shapegan_hip.h).
//
// SURVEY.md 8b asks for "a CPU twin (`*_cpu`) of each [entry point] for the no-GPU config and unit tests"; BASELINE configs[0]
// is `train_autoencoder.py classic ... on CPU (plumbing, no GPU)`.  Every function here is `sg_<name>_cpu` with the argument
// list of `sg_<name>` (the stream and workspace arguments are accepted and ignored; pointers are host pointers).  It is a
// SEPARATE implementation written against the header's contracts — straightforward loops with OpenMP over the outer index,
// no tiling heroics: correctness plumbing, not a performance path — and it shares no code with oracle/ (test infrastructure).
// With the HIP kernels it shares the per-element arithmetic of the areas that promise equal bits (csrc/*_core.h, mc_tables.h): one
// statement of each formula, the loops and summations around them written here.  Independence of those areas comes from the float64
// references of the tests (tests/geometry_reference.py, evaluation_reference.py, emd_reference.py), written from the header alone.
// The Python shells pick the twin only for tensors that live on the CPU (shapegan_amd/lib.py); GPU tensors never come here and
// there is no fallback in either direction.
//
// Opaque-buffer contracts it keeps compatible with the sizes the HIP library reports (host-side helpers, callable without a
// GPU): sg_sdfnet_packed_floats (this twin stores the plain weights at the front of the buffer), sg_sdfnet_bwd_blocks
// (bias partials: column 0 carries the row sums, the other columns zeros).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/shapegan_hip.h"   // the constants of the contract (SG_SDFNET_PARTIAL_ROW, SG_EMD_*, ...)

typedef void* hipStream_t_;
#define SG_OK 0          // csrc/common.h (the header names the codes only in its comments)
#define SG_ERR_ARG (-1)
#define SG_ERR_WORKSPACE (-3)
enum { ACT_NONE = 0, ACT_LEAKY = 1, ACT_RELU = 2, ACT_TANH = 3, ACT_SIGMOID = 4 };

static thread_local char g_err[512];
#define CPU_CHECK(cond)                                                                  \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            snprintf(g_err, sizeof(g_err), "%s: bad argument: %s", __func__, #cond);     \
            return SG_ERR_ARG;                                                           \
        }                                                                                \
    } while (0)

static inline float apply_act(float v, int act, float slope) {
    switch (act) {
        case ACT_LEAKY: return v > 0.f ? v : v * slope;
        case ACT_RELU: return v > 0.f ? v : 0.f;
        case ACT_TANH: return tanhf(v);
        case ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}
static inline float act_grad_out(float y, float dy, int act, float slope) {   // derivative through the activation OUTPUT
    switch (act) {
        case ACT_LEAKY: return y > 0.f ? dy : dy * slope;
        case ACT_RELU: return y > 0.f ? dy : 0.f;
        case ACT_TANH: return dy * (1.f - y * y);
        case ACT_SIGMOID: return dy * y * (1.f - y);
        default: return dy;
    }
}

extern "C" {

const char* sg_cpu_last_error(void) { return g_err; }

// ---- K1 / K2: Conv3d / ConvTranspose3d (kernel 4, stride 2, padding 1) ------------------------------------------------
int sg_conv3d_k4s2p1_fwd_cpu(const float* x, const float* w, const float* bias, float* y, int batch, int Cin, int Cin_total,
                             int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void*, size_t, void*) {
    CPU_CHECK(x && w && y && batch > 0 && Cin > 0 && Cin <= Cin_total && Cin <= Cx && Cout > 0 && !(ID & 1) && !(IH & 1) && !(IW & 1));
    const int OD = ID / 2, OH = IH / 2, OW = IW / 2;
    const long I3 = (long)ID * IH * IW, O3 = (long)OD * OH * OW;
#pragma omp parallel for collapse(2) schedule(static)
    for (int n = 0; n < batch; ++n)
        for (int co = 0; co < Cout; ++co) {
            float* yo = y + ((long)n * Cout + co) * O3;
            const float b = bias ? bias[co] : 0.f;
            for (long e = 0; e < O3; ++e) yo[e] = b;
            for (int ci = 0; ci < Cin; ++ci) {
                const float* xi = x + ((long)n * Cx + ci) * I3;
                const float* wk = w + ((long)co * Cin_total + ci) * 64;
                for (int kd = 0; kd < 4; ++kd)
                    for (int kh = 0; kh < 4; ++kh)
                        for (int kw = 0; kw < 4; ++kw) {
                            const float wv = wk[kd * 16 + kh * 4 + kw];
                            const int ow0 = kw == 0 ? 1 : 0, ow1 = kw == 3 ? OW - 1 : OW;   // 0 <= 2ow + kw - 1 < IW
                            for (int od = 0; od < OD; ++od) {
                                const int id = 2 * od + kd - 1;
                                if ((unsigned)id >= (unsigned)ID) continue;
                                for (int oh = 0; oh < OH; ++oh) {
                                    const int ih = 2 * oh + kh - 1;
                                    if ((unsigned)ih >= (unsigned)IH) continue;
                                    const float* xr = xi + ((long)id * IH + ih) * IW + kw - 1;
                                    float* yr = yo + ((long)od * OH + oh) * OW;
                                    for (int ow = ow0; ow < ow1; ++ow) yr[ow] += wv * xr[2 * ow];
                                }
                            }
                        }
            }
            if (act != ACT_NONE)
                for (long e = 0; e < O3; ++e) yo[e] = apply_act(yo[e], act, slope);
        }
    return SG_OK;
}

int sg_conv3d_k4s2p1_dgrad_cpu(const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin,
                               int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void*, size_t,
                               void*) {
    CPU_CHECK(dy && w && dx && batch > 0 && Cin > 0 && Cin <= Cin_total && Cin <= Cx && Cout > 0 && !(ID & 1) && !(IH & 1) && !(IW & 1));
    const int OD = ID / 2, OH = IH / 2, OW = IW / 2;
    const long I3 = (long)ID * IH * IW, O3 = (long)OD * OH * OW;
#pragma omp parallel for collapse(2) schedule(static)
    for (int n = 0; n < batch; ++n)
        for (int ci = 0; ci < Cin; ++ci) {
            float* xo = dx + ((long)n * Cx + ci) * I3;
            const float b = bias ? bias[ci] : 0.f;
            for (long e = 0; e < I3; ++e) xo[e] = b;
            for (int co = 0; co < Cout; ++co) {
                const float* yo = dy + ((long)n * Cout + co) * O3;
                const float* wk = w + ((long)co * Cin_total + ci) * 64;
                for (int kd = 0; kd < 4; ++kd)
                    for (int kh = 0; kh < 4; ++kh)
                        for (int kw = 0; kw < 4; ++kw) {
                            const float wv = wk[kd * 16 + kh * 4 + kw];
                            const int ow0 = kw == 0 ? 1 : 0, ow1 = kw == 3 ? OW - 1 : OW;
                            for (int od = 0; od < OD; ++od) {
                                const int id = 2 * od + kd - 1;
                                if ((unsigned)id >= (unsigned)ID) continue;
                                for (int oh = 0; oh < OH; ++oh) {
                                    const int ih = 2 * oh + kh - 1;
                                    if ((unsigned)ih >= (unsigned)IH) continue;
                                    float* xr = xo + ((long)id * IH + ih) * IW + kw - 1;
                                    const float* yr = yo + ((long)od * OH + oh) * OW;
                                    for (int ow = ow0; ow < ow1; ++ow) xr[2 * ow] += wv * yr[ow];
                                }
                            }
                        }
            }
            if (act != ACT_NONE)
                for (long e = 0; e < I3; ++e) xo[e] = apply_act(xo[e], act, slope);
        }
    return SG_OK;
}

int sg_conv3d_k4s2p1_wgrad_cpu(const float* dy, const float* x, float* dw, int batch, int Cin, int Cin_total, int Cx, int Cout,
                               int ID, int IH, int IW, void*, size_t, void*) {
    CPU_CHECK(dy && x && dw && batch > 0 && Cin > 0 && Cin <= Cin_total && Cin <= Cx && Cout > 0 && !(ID & 1) && !(IH & 1) && !(IW & 1));
    const int OD = ID / 2, OH = IH / 2, OW = IW / 2;
    const long I3 = (long)ID * IH * IW, O3 = (long)OD * OH * OW;
#pragma omp parallel for collapse(2) schedule(static)
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
            double acc[64];
            for (int k = 0; k < 64; ++k) acc[k] = 0.0;
            for (int n = 0; n < batch; ++n) {
                const float* yo = dy + ((long)n * Cout + co) * O3;
                const float* xi = x + ((long)n * Cx + ci) * I3;
                for (int kd = 0; kd < 4; ++kd)
                    for (int kh = 0; kh < 4; ++kh)
                        for (int kw = 0; kw < 4; ++kw) {
                            const int ow0 = kw == 0 ? 1 : 0, ow1 = kw == 3 ? OW - 1 : OW;
                            float s = 0.f;
                            for (int od = 0; od < OD; ++od) {
                                const int id = 2 * od + kd - 1;
                                if ((unsigned)id >= (unsigned)ID) continue;
                                for (int oh = 0; oh < OH; ++oh) {
                                    const int ih = 2 * oh + kh - 1;
                                    if ((unsigned)ih >= (unsigned)IH) continue;
                                    const float* xr = xi + ((long)id * IH + ih) * IW + kw - 1;
                                    const float* yr = yo + ((long)od * OH + oh) * OW;
                                    float r = 0.f;
                                    for (int ow = ow0; ow < ow1; ++ow) r += yr[ow] * xr[2 * ow];
                                    s += r;
                                }
                            }
                            acc[kd * 16 + kh * 4 + kw] += (double)s;
                        }
            }
            float* d = dw + ((long)co * Cin_total + ci) * 64;
            for (int k = 0; k < 64; ++k) d[k] = (float)acc[k];
        }
    return SG_OK;
}

int sg_conv3d_k4s2p1_dgrad_keep_cpu(const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin,
                                    int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void* ws,
                                    size_t wb, int, void* st) {     // (nothing is packed here: nothing to keep)
    return sg_conv3d_k4s2p1_dgrad_cpu(dy, w, bias, dx, batch, Cin, Cin_total, Cx, Cout, ID, IH, IW, act, slope, ws, wb, st);
}
int sg_conv3d_k4s2p1_dgrad_form_cpu(int, int, int, int, int, int, size_t) {     // (one loop nest serves every shape: no kernel forms here)
    return 0;      // SG_DGRAD_FORM_NONE
}
int sg_conv3d_k4s2p1_fwd_keep_cpu(const float* x, const float* w, const float* bias, float* y, int batch, int Cin, int Cin_total,
                                  int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void* ws, size_t wb, int, void* st) {
    return sg_conv3d_k4s2p1_fwd_cpu(x, w, bias, y, batch, Cin, Cin_total, Cx, Cout, ID, IH, IW, act, slope, ws, wb, st);
}
int sg_conv3d_k4s2p1_pack_images_cpu(int n, const int* kinds, const float* const* weights, void* const* workspaces,
                                     const size_t* workspace_bytes, const int* dims, int* served, void*) {
    CPU_CHECK(n > 0 && n <= 8 && kinds && weights && workspaces && workspace_bytes && dims && served);
    for (int i = 0; i < n; ++i) served[i] = 0;     // the twin reads the weights in place: there is no image to keep
    return SG_OK;
}
// (the twin's weight-gradient loops read dy in place: sg_conv3d_k4s2p1_wgrad_dy_image is a host query of the HIP library and
// answers for GPU tensors only; these two exist so that every entry point has its twin)
int sg_act_bwd_rowsum_pack8_cpu(const float* y, const float* dy, float* dz, float* rowsum, void*, long N, int C, long, int act,
                                float slope, void*) {
    CPU_CHECK(y && dy && dz && rowsum && N > 0 && C > 0);
    for (long r = 0; r < N * C; ++r) {
        double s = 0;
        for (int e = 0; e < 512; ++e) {
            const float v = act_grad_out(y[r * 512 + e], dy[r * 512 + e], act, slope);
            dz[r * 512 + e] = v;
            s += (double)v;
        }
        rowsum[r] = (float)s;
    }
    return SG_OK;
}
int sg_conv3d_k4s2p1_wgrad_prepacked_cpu(const float* dy, const float* x, float* dw, int batch, int Cin, int Cin_total, int Cx,
                                         int Cout, int ID, int IH, int IW, void* ws, size_t wb, void* st) {
    return sg_conv3d_k4s2p1_wgrad_cpu(dy, x, dw, batch, Cin, Cin_total, Cx, Cout, ID, IH, IW, ws, wb, st);
}
int sg_convT3d_k4s2p1_fwd_cpu(const float* x, const float* w, const float* bias, float* y, int batch, int Cin_T, int Cout_T,
                              int ID, int IH, int IW, int act, float slope, void* ws, size_t wb, void* st) {
    return sg_conv3d_k4s2p1_dgrad_cpu(x, w, bias, y, batch, Cout_T, Cout_T, Cout_T, Cin_T, 2 * ID, 2 * IH, 2 * IW, act, slope, ws,
                                      wb, st);
}
int sg_convT3d_k4s2p1_to1_pre_cpu(const float* x, const float* w, const float* bias, float* y, const float* in_scale,
                                  const float* in_shift, int in_act, float in_slope, int batch, int C, int ID, int IH, int IW,
                                  int act, float slope, void* st) {
    CPU_CHECK(x && w && y && in_scale && in_shift && batch > 0 && C > 0 && C <= 64 && IH * IW <= 256);
    CPU_CHECK(in_act == ACT_NONE || in_act == ACT_LEAKY || in_act == ACT_RELU);
    const long S = (long)ID * IH * IW, total = (long)batch * C * S;
    std::vector<float> t((size_t)total);
#pragma omp parallel for schedule(static)
    for (long e = 0; e < total; ++e) {
        const int c = (int)((e / S) % C);
        t[(size_t)e] = apply_act(x[e] * in_scale[c] + in_shift[c], in_act, in_slope);
    }
    return sg_conv3d_k4s2p1_dgrad_cpu(t.data(), w, bias, y, batch, 1, 1, 1, C, 2 * ID, 2 * IH, 2 * IW, act, slope, nullptr, 0, st);
}
int sg_convT3d_k4s2p1_to1_pre_grouped_cpu(const float* x, const float* w, const float* bias, float* y, const float* in_scale,
                                          const float* in_shift, int in_act, float in_slope, int batch, int C, int ID, int IH,
                                          int IW, int act, float slope, int spg, long y_group_stride, void* st) {
    CPU_CHECK(spg > 0 && batch % spg == 0);
    const long S = (long)ID * IH * IW;
    for (int g = 0; g < batch / spg; ++g) {
        const int rc = sg_convT3d_k4s2p1_to1_pre_cpu(x + (long)g * spg * C * S, w, bias, y + (long)g * y_group_stride,
                                                     in_scale + (long)g * C, in_shift + (long)g * C, in_act, in_slope, spg, C, ID, IH,
                                                     IW, act, slope, st);
        if (rc) return rc;
    }
    return SG_OK;
}
int sg_convT3d_k4s2p1_dgrad_cpu(const float* dy, const float* w, float* dx, int batch, int Cin_T, int Cout_T, int ID, int IH,
                                int IW, void* ws, size_t wb, void* st) {
    return sg_conv3d_k4s2p1_fwd_cpu(dy, w, nullptr, dx, batch, Cout_T, Cout_T, Cout_T, Cin_T, 2 * ID, 2 * IH, 2 * IW, ACT_NONE, 0.f,
                                    ws, wb, st);
}
int sg_convT3d_k4s2p1_wgrad_cpu(const float* dy, const float* x, float* dw, int batch, int Cin_T, int Cout_T, int ID, int IH,
                                int IW, void* ws, size_t wb, void* st) {
    return sg_conv3d_k4s2p1_wgrad_cpu(x, dy, dw, batch, Cout_T, Cout_T, Cout_T, Cin_T, 2 * ID, 2 * IH, 2 * IW, ws, wb, st);
}

// ---- K3 / K6: GEMM family -------------------------------------------------------------------------------------------------
int sg_gemm_cpu(const float* A, long sai, long sak, const float* B, long sbk, long sbj, float* C, long sci, long scj,
                const float* bias_i, const float* bias_j, int bias_j_shift, int M, int N, int K, int act, float slope, void*,
                size_t, void*) {
    CPU_CHECK(A && B && C && M > 0 && N > 0 && K > 0);
#pragma omp parallel for schedule(static)
    for (int i = 0; i < M; ++i) {
        std::vector<double> row(N, 0.0);
        for (int k = 0; k < K; ++k) {
            const double a = A[i * sai + k * sak];
            const float* bk = B + k * sbk;
            for (int j = 0; j < N; ++j) row[j] += a * (double)bk[j * sbj];
        }
        for (int j = 0; j < N; ++j) {
            float v = (float)row[j] + (bias_i ? bias_i[i] : 0.f) + (bias_j ? bias_j[j >> bias_j_shift] : 0.f);
            C[i * sci + j * scj] = apply_act(v, act, slope);
        }
    }
    return SG_OK;
}
int sg_gemm_nt_cpu(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, long K, void*, size_t,
                   void*) {
    CPU_CHECK(A && B && C && M > 0 && N > 0 && K > 0);
#pragma omp parallel for collapse(2) schedule(static)
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
            const float *a = A + i * lda, *b = B + j * ldb;
            double s = 0;
            for (long k = 0; k < K; ++k) s += (double)a[k] * (double)b[k];
            C[i * ldc + j] = (float)s;
        }
    return SG_OK;
}
int sg_gemm_nt_batched_cpu(const float* A, const long* a_off, long lda, const float* B, const long* b_off, long ldb, float* C,
                           const long* c_off, const long* ldc, int batch, int M, int N, long K, void* ws, size_t wb, void* st) {
    CPU_CHECK(A && B && C && a_off && b_off && c_off && ldc && batch > 0 && batch <= 8);
    for (int b = 0; b < batch; ++b) {
        const int rc = sg_gemm_nt_cpu(A + a_off[b], lda, B + b_off[b], ldb, C + c_off[b], ldc[b], M, N, K, ws, wb, st);
        if (rc) return rc;
    }
    return SG_OK;
}
int sg_gemm_nt_batched_lnrelu_cpu(const float* A, const long* a_off, long lda, const float* B, const long* b_off, long ldb,
                                  const float* gamma, const float* beta, const long* g_off, float* C, const long* c_off, const long* ldc,
                                  int batch, int M, int N, long K, void*, size_t, void*) {
    CPU_CHECK(A && B && C && a_off && b_off && c_off && ldc && gamma && beta && g_off && batch > 0 && batch <= 8 && M > 0 && N > 0 && K > 0);
    for (int m = 0; m < batch; ++m) {
        const float *Am = A + a_off[m], *Bm = B + b_off[m], *gm = gamma + g_off[m], *bt = beta + g_off[m];
        float* Cm = C + c_off[m];
#pragma omp parallel for collapse(2) schedule(static)
        for (int i = 0; i < M; ++i)
            for (int j = 0; j < N; ++j) {
                const float *a = Am + i * lda, *b = Bm + j * ldb;
                double s = 0;
                for (long k = 0; k < K; ++k) {
                    const float h = gm[j] * b[k] + bt[j];
                    s += (double)a[k] * (double)(h > 0.f ? h : 0.f);
                }
                Cm[i * ldc[m] + j] = (float)s;
            }
    }
    return SG_OK;
}
int sg_colsum_cpu(const float* x, float* out, int rows, int cols, long ld, void*) {
    CPU_CHECK(x && out && rows > 0 && cols > 0);
    for (int j = 0; j < cols; ++j) {
        double s = 0;
        for (int i = 0; i < rows; ++i) s += x[i * ld + j];
        out[j] = (float)s;
    }
    return SG_OK;
}
int sg_rowsum_cpu(const float* x, float* out, long rows, long len, long ld, void*) {
    CPU_CHECK(x && out && rows > 0 && len > 0);
#pragma omp parallel for schedule(static)
    for (long r = 0; r < rows; ++r) {
        double s = 0;
        for (long e = 0; e < len; ++e) s += x[r * ld + e];
        out[r] = (float)s;
    }
    return SG_OK;
}
int sg_rowsum_multi_cpu(const float* x, float* const* outs, const long* out_strides, int ndst, long rows_per_dst, long len,
                        long ld, void*) {
    CPU_CHECK(x && outs && ndst > 0 && ndst <= 8 && rows_per_dst > 0 && len > 0);
    for (int d = 0; d < ndst; ++d)
        for (long r = 0; r < rows_per_dst; ++r) {
            double s = 0;
            const float* p = x + ((long)d * rows_per_dst + r) * ld;
            for (long e = 0; e < len; ++e) s += p[e];
            outs[d][r * (out_strides ? out_strides[d] : 1)] = (float)s;
        }
    return SG_OK;
}
int sg_segsum_cpu(const float* x, float* out, long rows, long ld, const int64_t* seg_off, long nseg, void*) {
    CPU_CHECK(x && out && seg_off && rows > 0 && nseg > 0);
#pragma omp parallel for schedule(static)
    for (long r = 0; r < rows; ++r)
        for (long s = 0; s < nseg; ++s) {
            double acc = 0;
            for (long e = seg_off[s]; e < seg_off[s + 1]; ++e) acc += x[r * ld + e];
            out[r * nseg + s] = (float)acc;
        }
    return SG_OK;
}
int sg_colsum_tall_cpu(const float* x, float* out, long batch, long batch_stride, long rows, int cols, long ld, void*, size_t,
                       void*) {
    CPU_CHECK(x && out && batch > 0 && rows > 0 && cols > 0);
    for (long b = 0; b < batch; ++b)
        for (int c = 0; c < cols; ++c) {
            double s = 0;
            for (long r = 0; r < rows; ++r) s += x[b * batch_stride + r * ld + c];
            out[b * cols + c] = (float)s;
        }
    return SG_OK;
}

// ---- K4: BatchNorm ---------------------------------------------------------------------------------------------------------
#include "../csrc/batchnorm_core.h"
// the HIP launchers' plan, from the functions they share with this file (the loops below are plain: one pass per channel)
int sg_bn_plan_cpu(int N, int C, long S, int* nsplit, int* napply) {
    CPU_CHECK(nsplit && napply && N > 0 && C > 0 && S > 0);
    *nsplit = sg_bn_nsplit(N, C, S);
    *napply = sg_bn_apply_split(N, C, S);
    return SG_OK;
}
// The entries below walk a channel as the HIP kernels do (csrc/batchnorm.hip): the slices of sg_bn_plan, 256 lanes per slice with fp32
// sums of (x - K) and (x - K)^2 each, float4 groups where S % 4 == 0, the lanes' sums combined in double; the apply passes in `napply`
// slices.  A mistake in the slice arithmetic, the walk or the shift shows here as it would on the GPU.
namespace bn_twin {
// {sum(x-K), sum((x-K)^2)} of slice sp of channel c (bn_stats_kernel)
static void stats_slice(const float* x, int c, int N, int C, long S, int nsplit, int sp, double* out) {
    const long total = (long)N * S;
    long beg, end;
    sg_bn_slice(total, nsplit, sp, &beg, &end);
    const float K = sg_bn_shift(x, c, S);
    double d1 = 0, d2 = 0;
    for (int lane = 0; lane < 256; ++lane) {
        float s1 = 0.f, s2 = 0.f;
        if ((S & 3) == 0 && (beg & 3) == 0) {
            for (long e = beg + (long)lane * 4; e < end; e += 1024) {
                const float* v = x + sg_bn_chan_addr(e, c, C, S);
                const float a = v[0] - K, b = v[1] - K, cc = v[2] - K, d = v[3] - K;
                s1 += (a + b) + (cc + d);
                s2 += (a * a + b * b) + (cc * cc + d * d);
            }
        } else {
            for (long e = beg + lane; e < end; e += 256) {
                const float a = x[sg_bn_chan_addr(e, c, C, S)] - K;
                s1 += a;
                s2 += a * a;
            }
        }
        d1 += s1;
        d2 += s2;
    }
    out[0] = d1;
    out[1] = d2;
}
// mean, invstd and the biased variance of channel c from its nparts partials (bn_group_stats)
static void group_stats(const float* x, const double* partial, int c, int N, int C, long S, int nparts, float eps, float& mu, float& is,
                        double& var) {
    double s1 = 0, s2 = 0;
    for (int p = 0; p < nparts; ++p) {
        s1 += partial[p * 2];
        s2 += partial[p * 2 + 1];
    }
    const double n = (double)N * (double)S;
    double K = (double)sg_bn_shift(x, c, S);
    double m = s1 / n;
    var = s2 / n - m * m;
    if (var < 0) var = 0;
    if (sg_bn_shift_was_far(m, var)) {      // the statistics again around the mean the sums give, in double
        K = (double)(float)(K + m);
        const long total = (long)N * S;
        double t1 = 0, t2 = 0;
        for (long e = 0; e < total; ++e) {
            const double a = (double)x[sg_bn_chan_addr(e, c, C, S)] - K;
            t1 += a;
            t2 += a * a;
        }
        m = t1 / n;
        var = t2 / n - m * m;
        if (var < 0) var = 0;
    }
    mu = (float)(K + m);
    is = (float)(1.0 / sqrt(var + (double)eps));
}
// statistics of channel c and the running update (bn_update_running with one group)
static void channel_stats(const float* x, int c, int N, int C, long S, float eps, float momentum, float* running_mean, float* running_var,
                          float& mu, float& is) {
    const int ns = sg_bn_nsplit(N, C, S);
    double partial[64 * 2];
    for (int sp = 0; sp < ns; ++sp) stats_slice(x, c, N, C, S, ns, sp, partial + sp * 2);
    double var;
    group_stats(x, partial, c, N, C, S, ns, eps, mu, is, var);
    const double n = (double)N * (double)S;
    const double unbiased = n > 1 ? var * n / (n - 1) : var;
    if (running_mean) {
        running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
}
}  // namespace bn_twin

int sg_bn_train_fwd_cpu(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
                        float* running_mean, float* running_var, long long* num_batches_tracked, int N, int C, long S, float eps,
                        float momentum, int act, float slope, void*, size_t, void*) {
    CPU_CHECK(x && gamma && beta && y && save_mean && save_invstd && N > 0 && C > 0 && S > 0);
    const long total = (long)N * S;
    const int na = sg_bn_apply_split(N, C, S);
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        float mu, is;
        bn_twin::channel_stats(x, c, N, C, S, eps, momentum, running_mean, running_var, mu, is);
        save_mean[c] = mu;
        save_invstd[c] = is;
        // bn_finalize_apply_kernel's slices; the affine map in the centred form gamma ((x - mean) invstd) + beta, which does not lose
        // |mean| / std in the rounding of shift as the kernels' fma(x, scale, shift) does
        for (int sp = 0; sp < na; ++sp) {
            long beg, end;
            sg_bn_slice(total, na, sp, &beg, &end);
            if ((S & 3) == 0) {
                for (long e = beg; e < end; e += 4) {
                    const long ad = sg_bn_chan_addr(e, c, C, S);
                    for (int j = 0; j < 4; ++j) y[ad + j] = apply_act(gamma[c] * ((x[ad + j] - mu) * is) + beta[c], act, slope);
                }
            } else {
                for (long e = beg; e < end; ++e) {
                    const long ad = sg_bn_chan_addr(e, c, C, S);
                    y[ad] = apply_act(gamma[c] * ((x[ad] - mu) * is) + beta[c], act, slope);
                }
            }
        }
    }
    if (num_batches_tracked) *num_batches_tracked += 1;
    return SG_OK;
}
int sg_bn_train_stats_cpu(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float* scale, float* shift,
                          int N, int C, long S, float eps, float momentum, void*, size_t, void*) {
    CPU_CHECK(x && gamma && beta && save_mean && save_invstd && scale && shift && N > 0 && C > 0 && S > 0);
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        float mu, is;
        bn_twin::channel_stats(x, c, N, C, S, eps, momentum, running_mean, running_var, mu, is);
        save_mean[c] = mu;
        save_invstd[c] = is;
        scale[c] = gamma[c] * is;
        shift[c] = beta[c] - mu * scale[c];
    }
    if (num_batches_tracked) *num_batches_tracked += 1;
    return SG_OK;
}
int sg_bn_train_fwd_grouped_cpu(const float* x, const float* gamma, const float* beta, float* y, float* save_mean,
                                float* save_invstd, float* running_mean, float* running_var, long long* num_batches_tracked,
                                int groups, int N, int C, long S, float eps, float momentum, int act, float slope, void* ws, size_t wb,
                                void* st) {
    CPU_CHECK(groups > 0 && groups <= 64);
    for (int g = 0; g < groups; ++g) {     // the groups are independent batches, applied one after the other
        const long off = (long)g * N * C * S;
        const int rc = sg_bn_train_fwd_cpu(x + off, gamma, beta, y + off, save_mean + (long)g * C, save_invstd + (long)g * C,
                                           running_mean, running_var, num_batches_tracked, N, C, S, eps, momentum, act, slope, ws, wb,
                                           st);
        if (rc) return rc;
    }
    return SG_OK;
}
int sg_bn_train_stats_grouped_cpu(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                                  float* running_mean, float* running_var, long long* num_batches_tracked, float* scale,
                                  float* shift, int groups, int N, int C, long S, float eps, float momentum, void* ws, size_t wb,
                                  void* st) {
    CPU_CHECK(groups > 0 && groups <= 64);
    for (int g = 0; g < groups; ++g) {
        const int rc = sg_bn_train_stats_cpu(x + (long)g * N * C * S, gamma, beta, save_mean + (long)g * C, save_invstd + (long)g * C,
                                             running_mean, running_var, num_batches_tracked, scale + (long)g * C,
                                             shift + (long)g * C, N, C, S, eps, momentum, ws, wb, st);
        if (rc) return rc;
    }
    return SG_OK;
}
int sg_bn_eval_fwd_cpu(const float* x, const float* gamma, const float* beta, float* y, const float* running_mean,
                       const float* running_var, float* save_mean, float* save_invstd, int N, int C, long S, float eps, int act,
                       float slope, void*) {
    CPU_CHECK(x && gamma && beta && y && running_mean && running_var && save_mean && save_invstd && N > 0 && C > 0 && S > 0);
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        const float mu = running_mean[c], is = 1.f / sqrtf(running_var[c] + eps);
        save_mean[c] = mu;
        save_invstd[c] = is;
        for (int n = 0; n < N; ++n) {
            const float* p = x + ((long)n * C + c) * S;
            float* q = y + ((long)n * C + c) * S;
            for (long e = 0; e < S; ++e) q[e] = apply_act(gamma[c] * ((p[e] - mu) * is) + beta[c], act, slope);
        }
    }
    return SG_OK;
}
int sg_bn_bwd_cpu(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
                  const float* save_invstd, float* dx, float* dgamma, float* dbeta, int N, int C, long S, int train, int act,
                  float slope, void*, size_t, void*) {
    CPU_CHECK(dy && x && gamma && beta && save_mean && save_invstd && dx && dgamma && dbeta && N > 0 && C > 0 && S > 0);
    const long total = (long)N * S;
    const int ns = sg_bn_nsplit(N, C, S), na = sg_bn_apply_split(N, C, S);
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        const float mu = save_mean[c], is = save_invstd[c], g = gamma[c], b = beta[c];
        auto grad = [&](float xh, float d) { return act_grad_out(apply_act(fmaf(g, xh, b), act, slope), d, act, slope); };
        double t1 = 0, t2 = 0;
        for (int sp = 0; sp < ns; ++sp) {      // bn_bwd_stats_kernel: {sum(g), sum(g * xhat)}, two float4 groups in flight per lane
            long beg, end;
            sg_bn_slice(total, ns, sp, &beg, &end);
            for (int lane = 0; lane < 256; ++lane) {
                float s1 = 0.f, s2 = 0.f;
                if ((S & 3) == 0 && (beg & 3) == 0) {
                    SgChanWalk w(beg + (long)lane * 4, c, C, S);
                    long e = beg + (long)lane * 4;
                    for (; e + 1024 < end; e += 2048) {
                        const long a0 = w.addr();
                        w.advance(1024);
                        const long a1 = w.addr();
                        w.advance(1024);
                        for (int j = 0; j < 4; ++j) {
                            const float xh0 = (x[a0 + j] - mu) * is, xh1 = (x[a1 + j] - mu) * is;
                            const float g0 = grad(xh0, dy[a0 + j]), g1 = grad(xh1, dy[a1 + j]);
                            s1 += g0 + g1;
                            s2 += g0 * xh0 + g1 * xh1;
                        }
                    }
                    if (e < end) {
                        const long a0 = w.addr();
                        for (int j = 0; j < 4; ++j) {
                            const float xh0 = (x[a0 + j] - mu) * is;
                            const float g0 = grad(xh0, dy[a0 + j]);
                            s1 += g0;
                            s2 += g0 * xh0;
                        }
                    }
                } else {
                    for (long e = beg + lane; e < end; e += 256) {
                        const long ad = sg_bn_chan_addr(e, c, C, S);
                        const float xh = (x[ad] - mu) * is;
                        const float gg = grad(xh, dy[ad]);
                        s1 += gg;
                        s2 += gg * xh;
                    }
                }
                t1 += s1;
                t2 += s2;
            }
        }
        dbeta[c] = (float)t1;
        dgamma[c] = (float)t2;
        const float inv_n = 1.f / ((float)N * (float)S);
        const float db = (float)t1 * inv_n, dg = (float)t2 * inv_n;
        for (int sp = 0; sp < na; ++sp) {      // bn_bwd_finalize_apply_kernel
            long beg, end;
            sg_bn_slice(total, na, sp, &beg, &end);
            if ((S & 3) == 0 && (beg & 3) == 0) {
                for (int lane = 0; lane < 256; ++lane) {
                    SgChanWalk w(beg + (long)lane * 4, c, C, S);
                    for (long e = beg + (long)lane * 4; e < end; e += 1024) {
                        const long ad = w.addr();
                        w.advance(1024);
                        for (int j = 0; j < 4; ++j) {
                            const float xh = (x[ad + j] - mu) * is;
                            const float gg = grad(xh, dy[ad + j]);
                            dx[ad + j] = g * is * (train ? gg - db - xh * dg : gg);
                        }
                    }
                }
                continue;
            }
            for (long e = beg; e < end; ++e) {
                const long ad = sg_bn_chan_addr(e, c, C, S);
                const float xh = (x[ad] - mu) * is;
                const float gg = grad(xh, dy[ad]);
                dx[ad] = g * is * (train ? gg - db - xh * dg : gg);
            }
        }
    }
    return SG_OK;
}

// ---- K5: activations ---------------------------------------------------------------------------------------------------------
int sg_act_fwd_cpu(const float* x, float* y, long n, int act, float slope, void*) {
    CPU_CHECK(x && y && n > 0);
#pragma omp parallel for schedule(static)
    for (long e = 0; e < n; ++e) y[e] = apply_act(x[e], act, slope);
    return SG_OK;
}
int sg_act_bwd_cpu(const float* y, const float* dy, float* dx, long n, int act, float slope, void*) {
    CPU_CHECK(y && dy && dx && n > 0);
#pragma omp parallel for schedule(static)
    for (long e = 0; e < n; ++e) dx[e] = act_grad_out(y[e], dy[e], act, slope);
    return SG_OK;
}
int sg_act_bwd_rowsum_cpu(const float* y, const float* dy, float* dx, float* rowsum, long rows, long S, int act, float slope, void*) {
    CPU_CHECK(y && dy && dx && rowsum && rows > 0 && S > 0);
#pragma omp parallel for schedule(static)
    for (long r = 0; r < rows; ++r) {
        double s = 0;
        for (long e = r * S; e < (r + 1) * S; ++e) {
            dx[e] = act_grad_out(y[e], dy[e], act, slope);
            s += dx[e];
        }
        rowsum[r] = (float)s;
    }
    return SG_OK;
}
// weight + bias gradient through the activation (header: sg_conv3d_k4s2p1_wgrad_act): dz = dy * act'(y), then the plain forms
int sg_conv3d_k4s2p1_wgrad_act_cpu(const float* dy, const float* y, const float* x, float* dw, float* db, int batch, int Cin,
                                   int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void*, size_t,
                                   void*) {
    CPU_CHECK(dy && y && x && dw && db && batch > 0 && Cout > 0 && !(ID & 1) && !(IH & 1) && !(IW & 1));
    const long O3 = (long)(ID / 2) * (IH / 2) * (IW / 2), n = (long)batch * Cout * O3;
    std::vector<float> dz((size_t)n);
    for (long e = 0; e < n; ++e) dz[e] = act_grad_out(y[e], dy[e], act, slope);
    for (int co = 0; co < Cout; ++co) {
        double t = 0;
        for (int b = 0; b < batch; ++b)
            for (long e = 0; e < O3; ++e) t += dz[((long)b * Cout + co) * O3 + e];
        db[co] = (float)t;
    }
    return sg_conv3d_k4s2p1_wgrad_cpu(dz.data(), x, dw, batch, Cin, Cin_total, Cx, Cout, ID, IH, IW, nullptr, 0, nullptr);
}
int sg_act_bwd_dy_cpu(const float* y, const float* dy, const float* ggx, float* out, long n, int act, void*) {
    CPU_CHECK(y && dy && ggx && out && n > 0 && (act == ACT_TANH || act == ACT_SIGMOID));
    for (long e = 0; e < n; ++e) out[e] = ggx[e] * dy[e] * (act == ACT_TANH ? -2.f * y[e] : 1.f - 2.f * y[e]);
    return SG_OK;
}

// ---- K7: SDFNet ------------------------------------------------------------------------------------------------------------
// packed buffer of this twin (all row-major): W1k [256][KU] | W2 W3 W4 [256][256] | W5x [256][256] | W5i [256][KU] | W6 W7 |
// w8 [256] | b1..b7 [7][256] | b8
struct CpuSdf {
    int KU;
    const float *W1k, *W2, *W3, *W4, *W5x, *W5i, *W6, *W7, *w8, *b, *b8;
};
static CpuSdf sdf_view(const float* p, int KU) {
    CpuSdf v;
    v.KU = KU;
    v.W1k = p;
    p += 256L * KU;
    v.W2 = p; p += 65536;
    v.W3 = p; p += 65536;
    v.W4 = p; p += 65536;
    v.W5x = p; p += 65536;
    v.W5i = p; p += 256L * KU;
    v.W6 = p; p += 65536;
    v.W7 = p; p += 65536;
    v.w8 = p; p += 256;
    v.b = p; p += 7 * 256;
    v.b8 = p;
    return v;
}
int sg_sdfnet_pack_cpu(const float* const* params, int latent, int kin_used, float* packed, void*) {
    CPU_CHECK(params && packed && latent >= 0 && kin_used >= 3 && kin_used <= 3 + latent);
    const int kin = 3 + latent;
    float* p = packed;
    for (int o = 0; o < 256; ++o) memcpy(p + (long)o * kin_used, params[0] + (long)o * kin, sizeof(float) * kin_used);
    p += 256L * kin_used;
    for (int l = 1; l <= 3; ++l, p += 65536) memcpy(p, params[2 * l], sizeof(float) * 65536);
    for (int o = 0; o < 256; ++o) memcpy(p + o * 256, params[8] + (long)o * (256 + kin), sizeof(float) * 256);
    p += 65536;
    for (int o = 0; o < 256; ++o) memcpy(p + (long)o * kin_used, params[8] + (long)o * (256 + kin) + 256, sizeof(float) * kin_used);
    p += 256L * kin_used;
    for (int l = 5; l <= 6; ++l, p += 65536) memcpy(p, params[2 * l], sizeof(float) * 65536);
    memcpy(p, params[14], sizeof(float) * 256);
    p += 256;
    for (int l = 0; l < 7; ++l, p += 256) memcpy(p, params[2 * l + 1], sizeof(float) * 256);
    p[0] = params[15][0];
    return SG_OK;
}
// out[o] = relu?(b[o] + sum_k W[o][k] in[k]) for one point
static inline void dense(const float* W, int K, const float* in, const float* b, float* out, bool relu, bool accumulate) {
    for (int o = 0; o < 256; ++o) {
        const float* w = W + (long)o * K;
        float s = accumulate ? out[o] : (b ? b[o] : 0.f);
        for (int k = 0; k < K; ++k) s += w[k] * in[k];
        out[o] = s;
    }
    if (relu)
        for (int o = 0; o < 256; ++o) out[o] = out[o] > 0.f ? out[o] : 0.f;
}
int sg_sdfnet_fwd_cpu(const float* points, long points_period, const float* latent, const int64_t* latent_idx, int latent_size,
                      const float* packed, int kin_used, const float* zb1, const float* zb5, long points_per_shape,
                      const int* shape_index, float* out, float* acts, long ldn, long N, void*) {
    CPU_CHECK(points && packed && out && N > 0 && kin_used >= 3 && (kin_used == 3 || latent) && ((zb1 != nullptr) == (zb5 != nullptr)));
    // (the HIP library's rule — its tiles must not straddle shapes —, kept here so that the CPU tier sees a caller that breaks it)
    CPU_CHECK(!zb1 || shape_index || (points_per_shape > 0 && (points_per_shape % 128 == 0 || points_per_shape >= N)));
    const CpuSdf v = sdf_view(packed, kin_used);
    const int KU = kin_used, L = latent_size;
#pragma omp parallel for schedule(static)
    for (long p = 0; p < N; ++p) {
        float xin[3 + 1024], h[256], h2[256];
        const long pi = points_period > 0 ? p % points_period : p;
        for (int c = 0; c < 3; ++c) xin[c] = points[pi * 3 + c];
        if (KU > 3) {
            const long row = latent_idx ? latent_idx[p] : p;
            for (int k = 0; k < KU - 3; ++k) xin[3 + k] = latent[row * L + k];
        }
        const long shape = zb1 ? (shape_index ? shape_index[p] : p / points_per_shape) : 0;
        auto save = [&](int layer, const float* a) {
            if (acts)
                for (int o = 0; o < 256; ++o) acts[((long)layer * 256 + o) * ldn + p] = a[o];
        };
        dense(v.W1k, KU, xin, zb1 ? zb1 + shape * 256 : v.b, h, true, false);
        save(0, h);
        dense(v.W2, 256, h, v.b + 256, h2, true, false);
        save(1, h2);
        dense(v.W3, 256, h2, v.b + 512, h, true, false);
        save(2, h);
        dense(v.W4, 256, h, v.b + 768, h2, true, false);
        save(3, h2);
        dense(v.W5x, 256, h2, zb5 ? zb5 + shape * 256 : v.b + 1024, h, false, false);
        dense(v.W5i, KU, xin, nullptr, h, true, true);
        save(4, h);
        dense(v.W6, 256, h, v.b + 1280, h2, true, false);
        save(5, h2);
        dense(v.W7, 256, h2, v.b + 1536, h, true, false);
        save(6, h);
        float s = v.b8[0];
        for (int k = 0; k < 256; ++k) s += v.w8[k] * h[k];
        out[p] = tanhf(s);
    }
    return SG_OK;
}
// dH_in[k] = sum_o W[o][k] dZ[o]
static inline void dense_t(const float* W, int K, const float* dz, float* dh, bool accumulate) {
    if (!accumulate)
        for (int k = 0; k < K; ++k) dh[k] = 0.f;
    for (int o = 0; o < 256; ++o) {
        const float g = dz[o];
        if (g == 0.f) continue;
        const float* w = W + (long)o * K;
        for (int k = 0; k < K; ++k) dh[k] += w[k] * g;
    }
}
// ---- one point of one shape with frozen weights, per-shape bias mode (kin_used = 3): the latent fit, the projection, the sphere tracer
// weights of hidden layer l + 1, l = 1 .. 6 (its bias is v.b + 256 l; layer 5 takes zb5 and adds the point columns W5i instead)
static inline const float* sdf_hidden_w(const CpuSdf& v, int l) {
    const float* W[7] = {nullptr, v.W2, v.W3, v.W4, v.W5x, v.W6, v.W7};
    return W[l];
}
// the forward of sg_sdfnet_fwd_cpu for point x with the shape's bias rows (the same `dense` calls in the same order): h[l] = H_{l+1},
// returns the pre-activation of the last layer
static float sdf_shape_point_fwd(const CpuSdf& v, const float* x, const float* zb1_row, const float* zb5_row, float (*h)[256]) {
    dense(v.W1k, 3, x, zb1_row, h[0], true, false);
    for (int l = 1; l < 7; ++l) {
        if (l == 4) {
            dense(v.W5x, 256, h[3], zb5_row, h[4], false, false);
            dense(v.W5i, 3, x, nullptr, h[4], true, true);
        } else {
            dense(sdf_hidden_w(v, l), 256, h[l - 1], v.b + 256 * l, h[l], true, false);
        }
    }
    float pre = v.b8[0];
    for (int k = 0; k < 256; ++k) pre += v.w8[k] * h[6][k];
    return pre;
}
// the chain of sg_sdfnet_bwd_cpu from the upstream gradient d8 of the pre-activation, ReLU' read from h: leaves dZ1 in g and calls
// on_dz5(g) while g is dZ5
extern "C++" {      // (a template: not in the C-linkage block around it)
template <class OnDz5>
static void sdf_shape_point_chain(const CpuSdf& v, const float (*h)[256], float d8, float* g, OnDz5 on_dz5) {
    float gn[256];
    for (int r = 0; r < 256; ++r) g[r] = h[6][r] > 0.f ? v.w8[r] * d8 : 0.f;
    for (int layer = 5; layer >= 0; --layer) {
        dense_t(sdf_hidden_w(v, layer + 1), 256, g, gn, false);
        for (int r = 0; r < 256; ++r) g[r] = h[layer][r] > 0.f ? gn[r] : 0.f;
        if (layer == 4) on_dz5(g);
    }
}
// the chain and the point gradient gp[3] = W5[:, 256:259]^T dZ5 + W1[:, 0:3]^T dZ1 of its upstream gradient
template <class OnDz5>
static void sdf_shape_point_grad(const CpuSdf& v, const float (*h)[256], float d8, float* g, float* gp, OnDz5 on_dz5) {
    sdf_shape_point_chain(v, h, d8, g, [&](const float* dz5) {
        on_dz5(dz5);
        dense_t(v.W5i, 3, dz5, gp, false);
    });
    dense_t(v.W1k, 3, g, gp, true);
}
}
// the header's tile layout of the backward partials (sg_sdfnet_bwd_blocks / sg_sdfnet_bwd_tile_start)
static void sdf_bwd_plan(long N, long& nbig, long& nsmall) {
    const long tiles = (N + 63) / 64, rem = tiles % 512, full = tiles - rem;
    if (rem > 256 && rem <= 384) {
        nbig = full + 256;
        nsmall = (N - nbig * 64 + 31) / 32;
    } else if (full == 0 || rem == 0 || rem > 384) {
        nbig = tiles;
        nsmall = 0;
    } else {
        nbig = full;
        nsmall = (N - full * 64 + 31) / 32;
    }
}
static long sdf_bwd_tiles(long N) {
    long nbig, nsmall;
    sdf_bwd_plan(N, nbig, nsmall);
    return nbig + nsmall;
}
static long sdf_bwd_tile_start(long N, long t) {
    long nbig, nsmall;
    sdf_bwd_plan(N, nbig, nsmall);
    const long p = t <= nbig ? t * 64 : nbig * 64 + (t - nbig) * 32;
    return p < N ? p : N;
}
int sg_sdfnet_bwd_cpu(const float* dout, const float* out, const float* acts, float* dz, float* dz8, float* bias_partials,
                      const float* points, long points_period, float* dx, long dx_ld, const float* packed, int kin_used,
                      long ldn, long N, void*) {
    CPU_CHECK(dout && out && acts && dz && dz8 && packed && N > 0 && kin_used >= 3 && kin_used <= 3 + 1024);
    const CpuSdf v = sdf_view(packed, kin_used);
    const float* Wt[7] = {nullptr, v.W2, v.W3, v.W4, v.W5x, v.W6, v.W7};   // W of layer l+1 maps H_l -> Z_{l+1}
#pragma omp parallel for schedule(static)
    for (long p = 0; p < N; ++p) {
        float g[256], gn[256], dxa[3 + 1024];
        const float o = out[p];
        const float d8 = dout[p] * (1.f - o * o);
        dz8[p] = d8;
        auto masked_store = [&](int layer, float* gz) {
            for (int r = 0; r < 256; ++r) {
                gz[r] = acts[((long)layer * 256 + r) * ldn + p] > 0.f ? gz[r] : 0.f;
                dz[((long)layer * 256 + r) * ldn + p] = gz[r];
            }
        };
        for (int r = 0; r < 256; ++r) g[r] = v.w8[r] * d8;
        masked_store(6, g);
        for (int layer = 5; layer >= 0; --layer) {       // dH_layer = W_{layer+1}^T dZ_{layer+1}
            dense_t(Wt[layer + 1], 256, g, gn, false);
            if (dx && layer == 3) dense_t(v.W5i, kin_used, g, dxa, false);   // g is dZ5 here: the skip-connection input gradient
            memcpy(g, gn, sizeof(g));
            masked_store(layer, g);
        }
        if (dx) {
            dense_t(v.W1k, kin_used, g, dxa, true);
            for (int k = 0; k < kin_used; ++k) dx[p * dx_ld + k] = dxa[k];
        }
    }
    if (bias_partials) {
        // tile-major partial rows (header: SG_SDFNET_PARTIAL_ROW): 14 blocks of 256 row sums + the tile's sum of dz8
        const long nblk = sdf_bwd_tiles(N);
        const long nrows = points ? 14 * 256 : 7 * 256;
#pragma omp parallel for schedule(static)
        for (long t = 0; t < nblk; ++t) {
            const long p0 = sdf_bwd_tile_start(N, t), p1 = sdf_bwd_tile_start(N, t + 1);
            float* prow = bias_partials + t * SG_SDFNET_PARTIAL_ROW;
            for (long r = 0; r < nrows; ++r) {
                double s = 0;
                if (r < 7 * 256) {
                    for (long p = p0; p < p1; ++p) s += dz[r * ldn + p];
                } else if (r < 8 * 256) {                                   // w8 gradient: sum_p dz8[p] H7[row][p]
                    const long row = r - 7 * 256;
                    for (long p = p0; p < p1; ++p) s += (double)dz8[p] * acts[(6L * 256 + row) * ldn + p];
                } else {                                                    // point columns of dW1 (dZ1) / dW5 (dZ5)
                    const long q = r - 8 * 256, blk = q / (3 * 256), c = (q / 256) % 3, row = q % 256;
                    const long layer = blk == 0 ? 0 : 4;
                    for (long p = p0; p < p1; ++p) {
                        const long pi = points_period > 0 ? p % points_period : p;
                        s += (double)dz[(layer * 256 + row) * ldn + p] * points[pi * 3 + c];
                    }
                }
                prow[r] = (float)s;
            }
            double s8 = 0;
            for (long p = p0; p < p1; ++p) s8 += dz8[p];
            prow[14 * 256] = (float)s8;
        }
    }
    return SG_OK;
}
// the per-shape latent fold (header: sg_sdfnet_shape_bias)
int sg_sdfnet_shape_bias_cpu(const float* z, long nshapes, int latent, const float* W1, const float* b1, const float* W5,
                             const float* b5, float* zb1, float* zb5, void*) {
    CPU_CHECK(z && W1 && b1 && W5 && b5 && zb1 && zb5 && nshapes > 0 && latent > 0);
    const long ld1 = 3 + latent, ld5 = 259 + latent;
#pragma omp parallel for schedule(static)
    for (long e = 0; e < nshapes * 256; ++e) {
        const long s = e / 256, o = e % 256;
        double a = b1[o], b = b5[o];
        for (int k = 0; k < latent; ++k) {
            a += (double)z[s * latent + k] * W1[o * ld1 + 3 + k];
            b += (double)z[s * latent + k] * W5[o * ld5 + 259 + k];
        }
        zb1[e] = (float)a;
        zb5[e] = (float)b;
    }
    return SG_OK;
}
// backward of the per-shape latent fold (header: sg_sdfnet_shape_bias_bwd)
int sg_sdfnet_pack_shape_bias_cpu(const float* const* params, int latent, float* packed, const float* z, long nshapes, float* zb1,
                                  float* zb5, void* st) {
    CPU_CHECK(params && packed && latent > 0 && z && zb1 && zb5 && nshapes > 0);
    const int rc = sg_sdfnet_pack_cpu(params, latent, 3, packed, st);
    return rc ? rc : sg_sdfnet_shape_bias_cpu(z, nshapes, latent, params[0], params[1], params[8], params[9], zb1, zb5, st);
}
int sg_sdfnet_shape_bias_bwd_cpu(const float* t1, const float* t5, long nshapes, const float* z, int latent, const float* W1,
                                 const float* W5, float* dW1, float* dW5, float* gz, const float* reg_weight, float reg_scale, void*) {
    CPU_CHECK(t1 && t5 && z && W1 && W5 && nshapes > 0 && latent > 0 && (dW1 == nullptr) == (dW5 == nullptr));
    const long ld1 = 3 + latent, ld5 = 259 + latent;
    if (dW1) {
#pragma omp parallel for schedule(static)
        for (int o = 0; o < 256; ++o)
            for (int k = 0; k < latent; ++k) {
                double a = 0, b = 0;
                for (long s = 0; s < nshapes; ++s) {
                    a += (double)t1[o * nshapes + s] * z[s * latent + k];
                    b += (double)t5[o * nshapes + s] * z[s * latent + k];
                }
                dW1[o * ld1 + 3 + k] = (float)a;
                dW5[o * ld5 + 259 + k] = (float)b;
            }
    }
    if (gz) {
#pragma omp parallel for schedule(static)
        for (long s = 0; s < nshapes; ++s)
            for (int k = 0; k < latent; ++k) {
                double a = 0;
                for (int o = 0; o < 256; ++o)
                    a += (double)t1[o * nshapes + s] * W1[o * ld1 + 3 + k] + (double)t5[o * nshapes + s] * W5[o * ld5 + 259 + k];
                float v = (float)a;
                if (reg_scale != 0.f) v += ((reg_weight ? reg_weight[s] : 1.f) * reg_scale) * z[s * latent + k];
                gz[s * latent + k] = v;
            }
    }
    return SG_OK;
}
// the sums derived from one backward's partials (header: sg_sdfnet_bwd_finish): column sums over the tiles, segment sums
// straight from the images
int sg_sdfnet_bwd_finish_cpu(const float* dz, const float* bias_partials, long ldn, long N, int extended, float* const* bias_grads,
                             float* w8_grad, float* b8_grad, float* w1_cols, long w1_ld, float* w5_cols, long w5_ld,
                             const int64_t* seg_off, long nseg, float* t1, float* t5, void*, size_t, unsigned*, void*) {
    CPU_CHECK(dz && bias_partials && N > 0 && ldn >= N && nseg >= 0 && (!bias_grads || b8_grad));
    CPU_CHECK(!extended || !bias_grads || (w8_grad && w1_cols && w5_cols));
    CPU_CHECK(nseg == 0 || (seg_off && t1 && t5));
    const long nblk = sdf_bwd_tiles(N);
    if (bias_grads) {
        const int ngroups = extended ? 14 : 7;
#pragma omp parallel for schedule(static)
        for (long e = 0; e < (long)ngroups * 256; ++e) {
            const long g = e / 256, row = e % 256;
            double s = 0;
            for (long t = 0; t < nblk; ++t) s += bias_partials[t * SG_SDFNET_PARTIAL_ROW + e];
            if (g < 7)
                bias_grads[g][row] = (float)s;
            else if (g == 7)
                w8_grad[row] = (float)s;
            else if (g < 11)
                w1_cols[row * w1_ld + (g - 8)] = (float)s;
            else
                w5_cols[row * w5_ld + (g - 11)] = (float)s;
        }
        double s8 = 0;
        for (long t = 0; t < nblk; ++t) s8 += bias_partials[t * SG_SDFNET_PARTIAL_ROW + 14 * 256];
        b8_grad[0] = (float)s8;
    }
#pragma omp parallel for schedule(static)
    for (long pair = 0; pair < 256 * nseg; ++pair) {
        const long row = pair / nseg, sgm = pair % nseg;
        double a = 0, b = 0;
        for (long e = seg_off[sgm]; e < seg_off[sgm + 1]; ++e) {
            a += dz[row * ldn + e];
            b += dz[(4L * 256 + row) * ldn + e];
        }
        t1[pair] = (float)a;
        t5[pair] = (float)b;
    }
    return SG_OK;
}

// ---- K7c / K7e: loss and latent-only gradient with frozen weights, without and with a pose (header: sg_sdfnet_latent_grad /
// sg_sdfnet_latent_reduce, sg_sdfnet_latent_pose_grad / sg_sdfnet_latent_pose_reduce; csrc/latent_fit.hip) ------------------------------
// Per tile of the caller's table: the forward of sg_sdfnet_fwd_cpu point by point (the same `dense` calls in the same order, so a
// target made by that forward gives d == 0 exactly), the upstream gradient of the header, the chain of sg_sdfnet_bwd_cpu, and the
// tile's row sums of dZ1 / dZ5 and sum of |d|.  With a pose the same loop at x = A q + t (the header's fma order) with target' =
// clamp(ts target), and the point gradient as in sg_sdfnet_project_cpu, contracted with q per tile in point order.  Without one x is
// the point itself: one body, so the identity pose with ts = 1 gives floats [0, 513) of the row without a pose bit for bit.
extern "C++" {
template <bool POSE>
static void sdf_latent_grad_tiles(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                                  const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                                  long win_count, const int* tiles, long ntiles, float* partials) {
    constexpr int ROW = POSE ? SG_SDFNET_POSE_PARTIAL_ROW : SG_SDFNET_LATENT_PARTIAL_ROW;
    const CpuSdf v = sdf_view(packed, 3);
#pragma omp parallel for schedule(dynamic)
    for (long t = 0; t < ntiles; ++t) {
        float* prow = partials + t * ROW;
        for (int e = 0; e < ROW; ++e) prow[e] = 0.f;
        const long s = tiles[2 * t], i0 = tiles[2 * t + 1];
        if (s < 0 || s >= nshapes || i0 < 0) continue;
        const long beg = seg_off[s], n = seg_off[s + 1] - beg;
        const long m = win_count <= 0 || win_count > n ? n : win_count;
        long cnt = m - i0;
        if (cnt > SG_SDFNET_LATENT_TILE) cnt = SG_SDFNET_LATENT_TILE;
        const float* ps = POSE ? pose + s * 16 : nullptr;
        double s1[256] = {0}, s5[256] = {0};
        float labs = 0.f, gq[9] = {0.f}, gs[3] = {0.f}, es = 0.f;
        for (long i = 0; i < cnt; ++i) {
            const long pi = beg + (win_start + i0 + i) % n;
            const float* q = points + pi * 3;
            float xp[3], h[7][256], g[256];
            if (POSE)
                for (int c = 0; c < 3; ++c)
                    xp[c] = fmaf(ps[4 * c], q[0], fmaf(ps[4 * c + 1], q[1], fmaf(ps[4 * c + 2], q[2], ps[4 * c + 3])));
            const float o = tanhf(sdf_shape_point_fwd(v, POSE ? xp : q, zb1 + s * 256, zb5 + s * 256, h));
            const float raw = target[pi], st = POSE ? ps[12] * raw : raw;
            const float tg = fminf(fmaxf(st, -cutoff), cutoff);
            const float d = o - tg;
            labs += fabsf(d);
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float d8 = sg * ((1.f - o * o) / (float)m);
            auto sum5 = [&](const float* dz5) {
                for (int r = 0; r < 256; ++r) s5[r] += dz5[r];
            };
            if (POSE) {
                float gp[3] = {0.f, 0.f, 0.f};
                if (st > -cutoff && st < cutoff) es += (-sg * raw) / (float)m;
                sdf_shape_point_grad(v, h, d8, g, gp, sum5);
                for (int c = 0; c < 3; ++c) {
                    for (int j = 0; j < 3; ++j) gq[3 * c + j] += gp[c] * q[j];
                    gs[c] += gp[c];
                }
            } else {
                sdf_shape_point_chain(v, h, d8, g, sum5);
            }
            for (int r = 0; r < 256; ++r) s1[r] += g[r];
        }
        for (int r = 0; r < 256; ++r) {
            prow[r] = (float)s1[r];
            prow[256 + r] = (float)s5[r];
        }
        prow[512] = labs;
        if (POSE) {
            for (int e = 0; e < 9; ++e) prow[513 + e] = gq[e];
            for (int c = 0; c < 3; ++c) prow[522 + c] = gs[c];
            prow[525] = es;
        }
    }
}
template <bool POSE>
static void sdf_latent_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                              float* t1, float* t5, float* loss, float* gpose) {
    constexpr int ROW = POSE ? SG_SDFNET_POSE_PARTIAL_ROW : SG_SDFNET_LATENT_PARTIAL_ROW;
#pragma omp parallel for schedule(static)
    for (long s = 0; s < nshapes; ++s) {
        const long ta = tile_off[s], tb = tile_off[s + 1];
        for (int r = 0; r < (POSE ? 512 + 16 : 512); ++r) {
            const int k = r - 512;      // float k of gpose, in pose's layout: rows of A_c0 A_c1 A_c2 t_c, then ts
            const int col = r < 512 ? r : k == 12 ? 525 : (k & 3) == 3 ? 522 + (k >> 2) : 513 + 3 * (k >> 2) + (k & 3);
            double a = 0;
            if (r < 512 + 13)
                for (long t = ta; t < tb; ++t) a += partials[t * ROW + col];
            if (r < 512)
                (r < 256 ? t1 : t5)[(long)(r & 255) * nshapes + s] = (float)a;
            else
                gpose[s * 16 + (r - 512)] = (float)a;
        }
        double l = 0;
        for (long t = ta; t < tb; ++t) l += partials[t * ROW + 512];
        const long n = seg_off[s + 1] - seg_off[s];
        const long m = win_count <= 0 || win_count > n ? n : win_count;
        loss[s] = (float)(l / (double)(m > 0 ? m : 1));
    }
}
}
int sg_sdfnet_latent_grad_cpu(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                              const float* zb5, const float* packed, float cutoff, long win_start, long win_count,
                              const int* tiles, long ntiles, float* partials, void*) {
    CPU_CHECK(points && target && seg_off && zb1 && zb5 && packed && tiles && partials);
    CPU_CHECK(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    for (long s = 0; s < nshapes; ++s) CPU_CHECK(seg_off[s + 1] - seg_off[s] >= 1);
    sdf_latent_grad_tiles<false>(points, target, seg_off, nshapes, zb1, zb5, packed, nullptr, cutoff, win_start, win_count, tiles, ntiles,
                                 partials);
    return SG_OK;
}
int sg_sdfnet_latent_reduce_cpu(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                                float* t1, float* t5, float* loss, void*) {
    CPU_CHECK(partials && tile_off && seg_off && t1 && t5 && loss && nshapes >= 1);
    sdf_latent_reduce<false>(partials, tile_off, seg_off, nshapes, win_count, t1, t5, loss, nullptr);
    return SG_OK;
}
int sg_sdfnet_latent_pose_grad_cpu(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                                   const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                                   long win_count, const int* tiles, long ntiles, float* partials, void*) {
    CPU_CHECK(points && target && seg_off && zb1 && zb5 && packed && pose && tiles && partials);
    CPU_CHECK(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    for (long s = 0; s < nshapes; ++s) CPU_CHECK(seg_off[s + 1] - seg_off[s] >= 1);
    sdf_latent_grad_tiles<true>(points, target, seg_off, nshapes, zb1, zb5, packed, pose, cutoff, win_start, win_count, tiles, ntiles,
                                partials);
    return SG_OK;
}
int sg_sdfnet_latent_pose_reduce_cpu(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes,
                                     long win_count, float* t1, float* t5, float* loss, float* gpose, void*) {
    CPU_CHECK(partials && tile_off && seg_off && t1 && t5 && loss && gpose && nshapes >= 1 && nshapes < (1L << 31));
    sdf_latent_reduce<true>(partials, tile_off, seg_off, nshapes, win_count, t1, t5, loss, gpose);
    return SG_OK;
}

// ---- K7b: the LayerNorm form (SDFGenerator, model/point_sdf_net.py:49-119; header: sg_sdfgen_*) ------------------------------------
// The LayerNorm vectors sit where sg_sdfgen_packed_norm_offset (host code of the HIP library, shared) says: float offsets of the
// HIP image's layout for kin_used = 3, far behind this twin's own 462 337 floats.
static const long kGenG = 809216, kGenBe = 811008;
int sg_sdfgen_pack_cpu(const float* const* params, const float* const* norm_params, float* packed, void* st) {
    CPU_CHECK(params && norm_params && packed);
    const int rc = sg_sdfnet_pack_cpu(params, 0, 3, packed, st);
    if (rc) return rc;
    for (int l = 0; l < 7; ++l) {
        memcpy(packed + kGenG + l * 256, norm_params[2 * l], sizeof(float) * 256);
        memcpy(packed + kGenBe + l * 256, norm_params[2 * l + 1], sizeof(float) * 256);
    }
    return SG_OK;
}
// x (256 pre-LayerNorm values) -> xhat, rstd; h = relu(gamma xhat + beta)
static inline float ln_relu(const float* x, const float* g, const float* b, float eps, float* xhat, float* h) {
    double m = 0;
    for (int o = 0; o < 256; ++o) m += x[o];
    m /= 256;
    double v = 0;
    for (int o = 0; o < 256; ++o) v += ((double)x[o] - m) * ((double)x[o] - m);
    const float rstd = (float)(1.0 / sqrt(v / 256 + (double)eps));
    for (int o = 0; o < 256; ++o) {
        xhat[o] = (float)((double)x[o] - m) * rstd;
        const float y = g[o] * xhat[o] + b[o];
        h[o] = y > 0.f ? y : 0.f;
    }
    return rstd;
}
int sg_sdfgen_fwd_cpu(const float* points, const float* packed, const float* zb1, const float* zb5, long points_per_shape,
                      const int* shape_index, float eps, float* out, float* acts, long ldn, long N, void*) {
    CPU_CHECK(points && packed && zb1 && zb5 && out && N > 0 && eps > 0.f);
    // (the HIP kernel's tiles must not straddle shapes without a shape index: the twin refuses the same calls)
    CPU_CHECK(shape_index || (points_per_shape > 0 && (points_per_shape % 128 == 0 || points_per_shape >= N)));
    CPU_CHECK(!acts || ldn >= N);
    const CpuSdf v = sdf_view(packed, 3);
    const float *G = packed + kGenG, *Be = packed + kGenBe;
    float* rstd_img = acts ? acts + 7L * 256 * ldn + 56L * ldn : nullptr;
#pragma omp parallel for schedule(static)
    for (long p = 0; p < N; ++p) {
        float x[256], xh[256], h[256];
        const float* xin = points + p * 3;
        const long shape = shape_index ? shape_index[p] : p / points_per_shape;
        auto norm = [&](int layer) {
            const float r = ln_relu(x, G + layer * 256, Be + layer * 256, eps, xh, h);
            if (acts) {
                for (int o = 0; o < 256; ++o) acts[((long)layer * 256 + o) * ldn + p] = xh[o];
                rstd_img[(long)layer * ldn + p] = r;
            }
        };
        dense(v.W1k, 3, xin, zb1 + shape * 256, x, false, false);
        norm(0);
        dense(v.W2, 256, h, v.b + 256, x, false, false);
        norm(1);
        dense(v.W3, 256, h, v.b + 512, x, false, false);
        norm(2);
        dense(v.W4, 256, h, v.b + 768, x, false, false);
        norm(3);
        dense(v.W5x, 256, h, zb5 + shape * 256, x, false, false);
        dense(v.W5i, 3, xin, nullptr, x, false, true);
        norm(4);
        dense(v.W6, 256, h, v.b + 1280, x, false, false);
        norm(5);
        dense(v.W7, 256, h, v.b + 1536, x, false, false);
        norm(6);
        float s = v.b8[0];
        for (int k = 0; k < 256; ++k) s += v.w8[k] * h[k];
        out[p] = s;
    }
    return SG_OK;
}
int sg_sdfgen_bwd_cpu(const float* dout, const float* acts, float* dz, float* dz8, float* partials, const float* points,
                      const float* packed, long ldn, long N, void*) {
    CPU_CHECK(dout && acts && dz && dz8 && partials && points && packed && N > 0 && ldn >= N);
    const CpuSdf v = sdf_view(packed, 3);
    const float *G = packed + kGenG, *Be = packed + kGenBe;
    const float* Wt[7] = {nullptr, v.W2, v.W3, v.W4, v.W5x, v.W6, v.W7};
    const float* rstd_img = acts + 7L * 256 * ldn + 56L * ldn;
    const long nblk = (N + 31) / 32;
#pragma omp parallel for schedule(static)
    for (long t = 0; t < nblk; ++t) {
        std::vector<double> acc(28 * 256, 0.0);      // the tile's partial row (blocks 0..13, then the 14 LayerNorm blocks)
        double s8 = 0;
        const long p0 = t * 32, p1 = p0 + 32 < N ? p0 + 32 : N;
        for (long p = p0; p < p1; ++p) {
            float g[256], gn[256];
            const float d8 = dout[p];
            dz8[p] = d8;
            s8 += d8;
            // dH of image `layer` in g -> dZ (through ReLU and LayerNorm), stored; the LayerNorm parameter sums
            auto through_norm = [&](int layer) {
                const float *gm = G + layer * 256, *bt = Be + layer * 256;
                const float rs = rstd_img[(long)layer * ldn + p];
                double m1 = 0, m2 = 0;
                float dyh[256];
                for (int r = 0; r < 256; ++r) {
                    const float xh = acts[((long)layer * 256 + r) * ldn + p];
                    const float dy = gm[r] * xh + bt[r] > 0.f ? g[r] : 0.f;
                    acc[(14 + layer) * 256 + r] += (double)dy * xh;
                    acc[(21 + layer) * 256 + r] += dy;
                    dyh[r] = dy * gm[r];
                    m1 += dyh[r];
                    m2 += (double)dyh[r] * xh;
                }
                m1 /= 256;
                m2 /= 256;
                for (int r = 0; r < 256; ++r) {
                    const float xh = acts[((long)layer * 256 + r) * ldn + p];
                    g[r] = (float)(rs * ((double)dyh[r] - m1 - (double)xh * m2));
                    dz[((long)layer * 256 + r) * ldn + p] = g[r];
                    acc[layer * 256 + r] += g[r];
                }
            };
            for (int r = 0; r < 256; ++r) {
                const float xh = acts[(6L * 256 + r) * ldn + p];
                const float y = G[6 * 256 + r] * xh + Be[6 * 256 + r];
                acc[7 * 256 + r] += (double)d8 * (y > 0.f ? y : 0.f);      // w8 gradient: sum_p dz8 H7
                g[r] = v.w8[r] * d8;
            }
            through_norm(6);
            for (int layer = 5; layer >= 0; --layer) {
                dense_t(Wt[layer + 1], 256, g, gn, false);
                if (layer == 3)
                    for (int c = 0; c < 3; ++c)
                        for (int r = 0; r < 256; ++r) acc[(11 + c) * 256 + r] += (double)g[r] * points[p * 3 + c];   // g = dZ5
                memcpy(g, gn, sizeof(g));
                through_norm(layer);
            }
            for (int c = 0; c < 3; ++c)
                for (int r = 0; r < 256; ++r) acc[(8 + c) * 256 + r] += (double)g[r] * points[p * 3 + c];           // g = dZ1
        }
        float* prow = partials + t * SG_SDFGEN_PARTIAL_ROW;
        for (int e = 0; e < 14 * 256; ++e) prow[e] = (float)acc[e];
        prow[14 * 256] = (float)s8;
        for (int e = 0; e < 14 * 256; ++e) prow[SG_SDFNET_PARTIAL_ROW + e] = (float)acc[14 * 256 + e];
    }
    return SG_OK;
}
int sg_sdfgen_bwd_finish_cpu(const float* dz, const float* partials, long ldn, long N, float* const* bias_grads, float* w8_grad,
                             float* b8_grad, float* w1_cols, long w1_ld, float* w5_cols, long w5_ld, float* const* norm_grads,
                             const int64_t* seg_off, long nseg, float* t1, float* t5, void*, size_t, unsigned*, void*) {
    CPU_CHECK(dz && partials && N > 0 && ldn >= N && nseg >= 0 && bias_grads && norm_grads && w8_grad && b8_grad && w1_cols && w5_cols);
    CPU_CHECK(nseg == 0 || (seg_off && t1 && t5));
    const long nblk = (N + 31) / 32;
#pragma omp parallel for schedule(static)
    for (long e = 0; e < 28L * 256; ++e) {
        const long g = e / 256, row = e % 256;
        const long src = g < 14 ? e : SG_SDFNET_PARTIAL_ROW + (e - 14 * 256);
        double s = 0;
        for (long t = 0; t < nblk; ++t) s += partials[t * SG_SDFGEN_PARTIAL_ROW + src];
        if (g < 7)
            bias_grads[g][row] = (float)s;
        else if (g == 7)
            w8_grad[row] = (float)s;
        else if (g < 11)
            w1_cols[row * w1_ld + (g - 8)] = (float)s;
        else if (g < 14)
            w5_cols[row * w5_ld + (g - 11)] = (float)s;
        else
            norm_grads[g - 14][row] = (float)s;
    }
    double s8 = 0;
    for (long t = 0; t < nblk; ++t) s8 += partials[t * SG_SDFGEN_PARTIAL_ROW + 14 * 256];
    b8_grad[0] = (float)s8;
#pragma omp parallel for schedule(static)
    for (long pair = 0; pair < 256 * nseg; ++pair) {
        const long row = pair / nseg, sgm = pair % nseg;
        double a = 0, b = 0;
        for (long e = seg_off[sgm]; e < seg_off[sgm + 1]; ++e) {
            a += dz[row * ldn + e];
            b += dz[(4L * 256 + row) * ldn + e];
        }
        t1[pair] = (float)a;
        t5[pair] = (float)b;
    }
    return SG_OK;
}

// ---- PointNet.nn1 + max as a selection pass (header: sg_pointnet_pack / sg_pointnet_select) -----------------------------------------
// packed buffer of this twin: the four weight matrices row-major, one after the other
int sg_pointnet_pack_cpu(const float* const* weights, float* packed, void*) {
    CPU_CHECK(weights && packed && weights[0] && weights[1] && weights[2] && weights[3]);
    const long n[4] = {64 * 4, 128 * 64, 256 * 128, 512 * 256};
    float* p = packed;
    for (int i = 0; i < 4; ++i, p += n[i - 1]) memcpy(p, weights[i], sizeof(float) * n[i]);
    return SG_OK;
}
int sg_pointnet_select_cpu(const float* x, const float* packed, const float* const* biases, long B, long P, float* out, int* idx,
                           void*, size_t, void*) {
    CPU_CHECK(x && packed && biases && out && idx && B > 0 && P > 0 && P % 32 == 0);
    const float *W1 = packed, *W2 = W1 + 256, *W3 = W2 + 8192, *W4 = W3 + 32768;
#pragma omp parallel for schedule(static)
    for (long b = 0; b < B; ++b) {
        std::vector<float> best(512, -INFINITY);
        std::vector<int> bp(512, 0);
        for (long p = 0; p < P; ++p) {
            const float* in = x + (b * P + p) * 4;
            float h1[64], h2[128], h3[256];
            for (int o = 0; o < 64; ++o) {
                float s = biases[0][o];
                for (int k = 0; k < 4; ++k) s += W1[o * 4 + k] * in[k];
                h1[o] = s > 0.f ? s : 0.f;
            }
            for (int o = 0; o < 128; ++o) {
                float s = biases[1][o];
                for (int k = 0; k < 64; ++k) s += W2[o * 64 + k] * h1[k];
                h2[o] = s > 0.f ? s : 0.f;
            }
            for (int o = 0; o < 256; ++o) {
                float s = biases[2][o];
                for (int k = 0; k < 128; ++k) s += W3[o * 128 + k] * h2[k];
                h3[o] = s > 0.f ? s : 0.f;
            }
            for (int o = 0; o < 512; ++o) {
                float s = biases[3][o];
                for (int k = 0; k < 256; ++k) s += W4[o * 256 + k] * h3[k];
                if (s > best[o]) best[o] = s, bp[o] = (int)p;
            }
        }
        for (int o = 0; o < 512; ++o) out[b * 512 + o] = best[o], idx[b * 512 + o] = bp[o];
    }
    return SG_OK;
}

// ---- K8 - K11: elementwise, reductions, table rows, optimizers ---------------------------------------------------------------
int sg_axpby_cpu(const float* x, const float* y, float* out, long n, float a, float b, void*) {
    CPU_CHECK(x && out && n > 0);
    for (long e = 0; e < n; ++e) out[e] = y ? a * x[e] + b * y[e] : a * x[e];
    return SG_OK;
}
int sg_reduce_sum_cpu(const float* x, float* out, long n, float scale, void*, size_t, void*) {
    CPU_CHECK(x && out && n > 0);
    double s = 0;
    for (long e = 0; e < n; ++e) s += x[e];
    out[0] = (float)(s * (double)scale);
    return SG_OK;
}
int sg_gather_rows_cpu(const float* table, const int64_t* idx, float* out, long n, int L, void*) {
    CPU_CHECK(table && idx && out && n > 0 && L > 0);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < n; ++i) memcpy(out + i * L, table + idx[i] * L, sizeof(float) * L);
    return SG_OK;
}
int sg_scatter_add_rows_cpu(const float* rows, long rows_ld, const int64_t* idx, float* table_grad, long n, int L, void*) {
    CPU_CHECK(rows && idx && table_grad && n > 0 && L > 0 && rows_ld >= L);
    for (long i = 0; i < n; ++i)
        for (int k = 0; k < L; ++k) table_grad[idx[i] * L + k] += rows[i * rows_ld + k];
    return SG_OK;
}
// stable counting sort of the batch on the shape id (header: sg_sdf_batch_sort)
int sg_sdf_batch_sort_cpu(const int64_t* indices, long n, long pointcloud_size, long nshapes, const float* points, const float* sdf,
                          float* out_points, float* out_sdf, int* out_shape, int64_t* seg_off, float* counts, int* bad_index_flag,
                          int* bad_index_device, int bad_index_value, void*, size_t, void*) {
    CPU_CHECK(indices && points && sdf && out_points && out_sdf && out_shape && seg_off && counts && bad_index_flag);
    CPU_CHECK(n > 0 && pointcloud_size > 0 && nshapes > 0 && bad_index_value != 0);
    std::vector<int64_t> next(nshapes + 1, 0);
    auto shape_of = [&](int64_t i) {
        int64_t k = i >= 0 ? i / pointcloud_size : -1;
        if (k < 0 || k >= nshapes) {
            if (!bad_index_device) {
                *bad_index_flag = bad_index_value;
            } else if (*bad_index_device == 0 || *bad_index_device == bad_index_value) {
                *bad_index_device = bad_index_value;
                *bad_index_flag = bad_index_value;
            }
            k = k < 0 ? 0 : nshapes - 1;
        }
        return k;
    };
    for (long e = 0; e < n; ++e) next[shape_of(indices[e]) + 1] += 1;
    for (long s = 0; s < nshapes; ++s) {
        counts[s] = (float)next[s + 1];
        next[s + 1] += next[s];
    }
    for (long s = 0; s <= nshapes; ++s) seg_off[s] = next[s];
    for (long e = 0; e < n; ++e) {
        const int64_t k = shape_of(indices[e]), p = next[k]++, rows = nshapes * pointcloud_size;
        const int64_t i = indices[e] < 0 ? 0 : (indices[e] < rows ? indices[e] : rows - 1);   // (flagged above)
        memcpy(out_points + p * 3, points + i * 3, 3 * sizeof(float));
        out_sdf[p] = sdf[i];
        out_shape[p] = (int)k;
    }
    return SG_OK;
}
int sg_rmsprop_step_cpu(float* p, const float* g, float* sq, long n, float lr, float alpha, float eps, float gscale, float clip, void*) {
    CPU_CHECK(p && g && sq && n > 0);
    for (long e = 0; e < n; ++e) {
        const float gg = g[e] * gscale;
        const float s = alpha * sq[e] + (1.f - alpha) * gg * gg;
        sq[e] = s;
        float v = p[e] - lr * (gg / (sqrtf(s) + eps));
        if (clip > 0.f) v = std::min(std::max(v, -clip), clip);
        p[e] = v;
    }
    return SG_OK;
}
static void adam_update(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float bc1,
                        float bc2_sqrt, float gscale) {
    const float step = lr / bc1;
    for (long e = 0; e < n; ++e) {
        const float gg = g[e] * gscale;
        const float mm = b1 * m[e] + (1.f - b1) * gg;
        const float vv = b2 * v[e] + (1.f - b2) * gg * gg;
        m[e] = mm;
        v[e] = vv;
        p[e] = p[e] - step * (mm / (sqrtf(vv) / bc2_sqrt + eps));
    }
}
int sg_adam_step_guarded_cpu(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                             long step, float gscale, const int* skip, void*) {
    CPU_CHECK(p && g && m && v && n > 0 && step > 0);
    if (skip && *skip) return SG_OK;
    adam_update(p, g, m, v, n, lr, b1, b2, eps, (float)(1.0 - pow((double)b1, (double)step)),
                (float)sqrt(1.0 - pow((double)b2, (double)step)), gscale);
    return SG_OK;
}
int sg_adam_step_cpu(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, long step,
                     float gscale, void* stream) {
    return sg_adam_step_guarded_cpu(p, g, m, v, n, lr, b1, b2, eps, step, gscale, nullptr, stream);
}
int sg_adam_step_dev_multi_cpu(int nsets, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                               const float* lr, const float* b1, const float* b2, const float* eps, long long* const* step_dev,
                               float* const* corr_dev, const float* gscale, const int* skip, void* stream);
int sg_adam_step_dev_guarded_cpu(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                                 long long* step_dev, float* corr_dev, float gscale, const int* skip, void*) {
    CPU_CHECK(p && g && m && v && n > 0 && step_dev && corr_dev);
    if (skip && *skip) return SG_OK;
    const long long t = ++*step_dev;
    corr_dev[0] = (float)(1.0 - pow((double)b1, (double)t));
    corr_dev[1] = (float)sqrt(1.0 - pow((double)b2, (double)t));
    adam_update(p, g, m, v, n, lr, b1, b2, eps, corr_dev[0], corr_dev[1], gscale);
    return SG_OK;
}
int sg_adam_step_dev_multi_cpu(int nsets, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                               const float* lr, const float* b1, const float* b2, const float* eps, long long* const* step_dev,
                               float* const* corr_dev, const float* gscale, const int* skip, void* stream) {
    CPU_CHECK(nsets > 0 && nsets <= 4 && p && g && m && v && n && lr && b1 && b2 && eps && step_dev && corr_dev && gscale);
    // (every set is looked at before the first is updated, as the library does before its one launch)
    for (int i = 0; i < nsets; ++i) CPU_CHECK(p[i] && g[i] && m[i] && v[i] && n[i] > 0 && step_dev[i] && corr_dev[i]);
    for (int i = 0; i < nsets; ++i) {
        const int rc = sg_adam_step_dev_guarded_cpu(p[i], g[i], m[i], v[i], n[i], lr[i], b1[i], b2[i], eps[i], step_dev[i], corr_dev[i],
                                                    gscale[i], skip, stream);
        if (rc) return rc;
    }
    return SG_OK;
}
int sg_adam_step_dev_cpu(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                         long long* step_dev, float* corr_dev, float gscale, void* stream) {
    return sg_adam_step_dev_guarded_cpu(p, g, m, v, n, lr, b1, b2, eps, step_dev, corr_dev, gscale, nullptr, stream);
}
int sg_clamp_cpu(float* p, long n, float lo, float hi, void*) {
    CPU_CHECK(p && n > 0);
    for (long e = 0; e < n; ++e) p[e] = std::min(std::max(p[e], lo), hi);
    return SG_OK;
}
int sg_clamp_multi_cpu(float* const* tensors, const long* counts, int ntensors, float lo, float hi, void*) {
    CPU_CHECK(tensors && counts && ntensors > 0);
    for (int i = 0; i < ntensors; ++i) {
        const int rc = sg_clamp_cpu(tensors[i], counts[i], lo, hi, nullptr);
        if (rc != SG_OK) return rc;
    }
    return SG_OK;
}
int sg_voxel_prepare_cpu(const float* x, float* out, long n, float c, float divisor, void*) {
    CPU_CHECK(x && out && n > 0 && c >= 0.f);
    for (long e = 0; e < n; ++e) {
        float v = x[e];
        v = v < -c ? -c : (v > c ? c : v);
        out[e] = divisor > 0.f ? v / divisor : v;
    }
    return SG_OK;
}

// ---- losses / blends ----------------------------------------------------------------------------------------------------------
int sg_loss_weighted_l1_fwd_cpu(const float* o, const float* t, long n, float negw, float* loss, void*, size_t, void*) {
    CPU_CHECK(o && t && loss && n > 0);
    double s = 0;
    for (long e = 0; e < n; ++e) s += fabs((double)((o[e] - t[e]) * (t[e] < 0.f ? negw : 1.f)));
    loss[0] = (float)(s / (double)n);
    return SG_OK;
}
int sg_loss_weighted_l1_bwd_cpu(const float* o, const float* t, const float* gloss, float* d_o, long n, float negw, void*) {
    CPU_CHECK(o && t && gloss && d_o && n > 0);
    const float g = gloss[0] * (float)(1.0 / (double)n);
    for (long e = 0; e < n; ++e) {
        const float w = t[e] < 0.f ? negw : 1.f, d = (o[e] - t[e]) * w;
        d_o[e] = g * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * w;
    }
    return SG_OK;
}
int sg_count_sign_mismatch_cpu(const float* a, const float* b, long n, long long* count, void*, size_t, void*) {
    CPU_CHECK(a && b && count && n > 0);
    long long c = 0;
    for (long e = 0; e < n; ++e) {
        volatile float prod = a[e] * b[e];     // the rounded fp32 product, as `(input * target) < 0` sees it
        c += prod < 0.f ? 1 : 0;
    }
    count[0] = c;
    return SG_OK;
}
int sg_loss_mean_split_fwd_cpu(const float* x, long n, long n_first, float w_first, float w_rest, float* loss, float* dx_unit,
                               void*) {
    CPU_CHECK(x && loss && n > 0 && n_first >= 0 && n_first <= n);
    if (dx_unit) {
        const float ca = n_first > 0 ? (float)((double)w_first / (double)n_first) : 0.f;
        const float cb = n > n_first ? (float)((double)w_rest / (double)(n - n_first)) : 0.f;
        for (long e = 0; e < n; ++e) dx_unit[e] = e < n_first ? ca : cb;
    }
    double a = 0, b = 0;
    for (long e = 0; e < n; ++e) (e < n_first ? a : b) += x[e];
    double v = 0;
    if (n_first > 0) v += (double)w_first * a / (double)n_first;
    if (n > n_first) v += (double)w_rest * b / (double)(n - n_first);
    loss[0] = (float)v;
    return SG_OK;
}
int sg_loss_mean_split_bwd_cpu(const float* gloss, float* dx, long n, long n_first, float w_first, float w_rest, void*) {
    CPU_CHECK(gloss && dx && n > 0 && n_first >= 0 && n_first <= n);
    const float ca = n_first > 0 ? (float)((double)w_first / (double)n_first) : 0.f;
    const float cb = n > n_first ? (float)((double)w_rest / (double)(n - n_first)) : 0.f;
    for (long e = 0; e < n; ++e) dx[e] = gloss[0] * (e < n_first ? ca : cb);
    return SG_OK;
}
// ---- classic-GAN losses on the [B] vector of discriminator outputs; VAE reparameterisation; the critic's last layer ---------
int sg_loss_bce_fwd_cpu(const float* p, long n, float t, float* loss, void*) {
    CPU_CHECK(p && loss && n > 0);
    double s = 0;
    for (long e = 0; e < n; ++e)
        s -= (double)(t * std::max(logf(p[e]), -100.f) + (1.f - t) * std::max(logf(1.f - p[e]), -100.f));
    loss[0] = (float)(s / (double)n);
    return SG_OK;
}
int sg_loss_bce_bwd_cpu(const float* p, const float* gloss, float* dp, long n, float t, void*) {
    CPU_CHECK(p && gloss && dp && n > 0);
    const float g = gloss[0] * (float)(1.0 / (double)n);
    for (long e = 0; e < n; ++e) dp[e] = g * (p[e] - t) / std::max((1.f - p[e]) * p[e], 1e-12f);
    return SG_OK;
}
int sg_loss_neg_mean_log_fwd_cpu(const float* p, long n, float* loss, void*) {
    CPU_CHECK(p && loss && n > 0);
    double s = 0;
    for (long e = 0; e < n; ++e) s -= (double)logf(p[e]);
    loss[0] = (float)(s / (double)n);
    return SG_OK;
}
int sg_loss_neg_mean_log_bwd_cpu(const float* p, const float* gloss, float* dp, long n, void*) {
    CPU_CHECK(p && gloss && dp && n > 0);
    const float g = gloss[0] * (float)(1.0 / (double)n);
    for (long e = 0; e < n; ++e) dp[e] = -g / p[e];
    return SG_OK;
}
int sg_vae_reparam_fwd_cpu(const float* mu, const float* lv, const float* eps, float* z, long n, void*) {
    CPU_CHECK(mu && lv && eps && z && n > 0);
    for (long e = 0; e < n; ++e) {
        const float sd = expf(lv[e] * 0.5f);
        volatile float prod = sd * eps[e];     // two roundings, as the reference's `mean + standard_deviation * eps`
        z[e] = mu[e] + prod;
    }
    return SG_OK;
}
int sg_vae_reparam_bwd_cpu(const float* lv, const float* eps, const float* gz, float* dlv, long n, void*) {
    CPU_CHECK(lv && eps && gz && dlv && n > 0);
    for (long e = 0; e < n; ++e) dlv[e] = gz[e] * eps[e] * (0.5f * expf(lv[e] * 0.5f));
    return SG_OK;
}
static inline float head_act_cpu(float v, int act, float slope) {
    return act == ACT_LEAKY ? (v > 0.f ? v : v * slope) : (act == ACT_RELU ? (v > 0.f ? v : 0.f) : v);
}
int sg_head_dot_fwd_cpu(const float* z, const float* w, const float* bias, float* y, int N, long K, int act, float slope, void*) {
    CPU_CHECK(z && w && y && N > 0 && K > 0 && K % 4 == 0);
    CPU_CHECK(act == ACT_NONE || act == ACT_LEAKY || act == ACT_RELU);
#pragma omp parallel for
    for (int n = 0; n < N; ++n) {
        double s = 0;
        for (long k = 0; k < K; ++k) s += (double)head_act_cpu(z[(long)n * K + k], act, slope) * (double)w[k];
        y[n] = (float)s + (bias ? bias[0] : 0.f);
    }
    return SG_OK;
}
int sg_head_dot_bwd_cpu(const float* z, const float* w, const float* gy, float* gz, float* gw, float* gb, float* gbz, void*, int N,
                        int C, int S, int act, float slope, void*) {
    CPU_CHECK(z && w && gy && gz && N > 0 && C > 0 && S == 64);
    CPU_CHECK(act == ACT_NONE || act == ACT_LEAKY || act == ACT_RELU);
    const long K = (long)C * S;
#pragma omp parallel for
    for (int c = 0; c < C; ++c) {
        double cz = 0;
        for (int s = 0; s < S; ++s) {
            const long k = (long)c * S + s;
            double aw = 0;
            for (int n = 0; n < N; ++n) {
                const float v = z[(long)n * K + k];
                const float d = act == ACT_LEAKY ? (v > 0.f ? 1.f : slope) : (act == ACT_RELU ? (v > 0.f ? 1.f : 0.f) : 1.f);
                const float o = gy[n] * w[k] * d;
                gz[(long)n * K + k] = o;
                cz += (double)o;
                aw += (double)gy[n] * (double)head_act_cpu(v, act, slope);
            }
            if (gw) gw[k] = (float)aw;
        }
        if (gbz) gbz[c] = (float)cz;
    }
    if (gb) {
        double t = 0;
        for (int n = 0; n < N; ++n) t += (double)gy[n];
        gb[0] = (float)t;
    }
    return SG_OK;
}
int sg_loss_kld_fwd_cpu(const float* mu, const float* lv, long n, float* loss, void*, size_t, void*) {
    CPU_CHECK(mu && lv && loss && n > 0);
    double s = 0;
    for (long e = 0; e < n; ++e) s += (double)(1.f + lv[e] - mu[e] * mu[e] - expf(lv[e]));
    loss[0] = (float)(-0.5 * s / (double)n);
    return SG_OK;
}
int sg_loss_kld_bwd_cpu(const float* mu, const float* lv, const float* gloss, float* dmu, float* dlv, long n, void*) {
    CPU_CHECK(mu && lv && gloss && dmu && dlv && n > 0);
    const float g = gloss[0] * (float)(1.0 / (double)n);
    for (long e = 0; e < n; ++e) {
        dmu[e] = g * mu[e];
        dlv[e] = -0.5f * g * (1.f - expf(lv[e]));
    }
    return SG_OK;
}
int sg_loss_meansq_fwd_cpu(const float* x, const float* roww, long rows, int L, double denom, float* loss, void*, size_t, void*) {
    CPU_CHECK(x && loss && rows > 0 && L > 0 && denom > 0);
    double s = 0;
    for (long e = 0; e < rows * L; ++e) s += (double)((roww ? roww[e / L] : 1.f) * x[e] * x[e]);
    loss[0] = (float)(s / denom);
    return SG_OK;
}
int sg_loss_meansq_bwd_cpu(const float* x, const float* roww, const float* gloss, float* dx, long rows, int L, double denom, void*) {
    CPU_CHECK(x && gloss && dx && rows > 0 && L > 0 && denom > 0);
    const float g = gloss[0] * (float)(2.0 / denom);
    for (long e = 0; e < rows * L; ++e) dx[e] = (roww ? roww[e / L] : 1.f) * g * x[e];
    return SG_OK;
}
int sg_loss_deepsdf_fwd_cpu(const float* o, const float* t, long n, const float* z, const float* roww, long rows, int L, double denom,
                            float* loss, void*, size_t, void*) {
    CPU_CHECK(o && t && z && loss && n > 0 && rows > 0 && L > 0 && denom > 0);
    double s1 = 0, s2 = 0;
    for (long e = 0; e < n; ++e) s1 += fabs((double)(o[e] - t[e]));
    for (long e = 0; e < rows * L; ++e) s2 += (double)((roww ? roww[e / L] : 1.f) * z[e] * z[e]);
    loss[0] = (float)(s1 / (double)n) + (float)(s2 / denom);
    return SG_OK;
}
int sg_loss_deepsdf_bwd_cpu(const float* o, const float* t, long n, const float* z, const float* roww, long rows, int L, double denom,
                            const float* gloss, float* d_o, float* dz, void*) {
    CPU_CHECK(o && t && z && gloss && d_o && dz && n > 0 && rows > 0 && L > 0 && denom > 0);
    const float g1 = gloss[0] * (float)(1.0 / (double)n), g2 = gloss[0] * (float)(2.0 / denom);
    for (long e = 0; e < n; ++e) {
        const float d = o[e] - t[e];
        d_o[e] = g1 * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
    for (long e = 0; e < rows * L; ++e) dz[e] = (roww ? roww[e / L] : 1.f) * g2 * z[e];
    return SG_OK;
}
int sg_loss_deepsdf_fused_cpu(const float* o, const float* t, long n, const float* z, const float* roww, long rows, int L, double denom,
                              float* loss, float* d_o, float* dz, void*, size_t, unsigned*, void*) {
    CPU_CHECK(o && t && z && loss && n > 0 && rows > 0 && L > 0 && denom > 0);
    const int rc = sg_loss_deepsdf_fwd_cpu(o, t, n, z, roww, rows, L, denom, loss, nullptr, 0, nullptr);
    if (rc != SG_OK) return rc;
    const float g1 = (float)(1.0 / (double)n), g2 = (float)(2.0 / denom);
    if (d_o)
        for (long e = 0; e < n; ++e) {
            const float d = o[e] - t[e];
            d_o[e] = g1 * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        }
    if (dz)
        for (long e = 0; e < rows * L; ++e) dz[e] = (roww ? roww[e / L] : 1.f) * g2 * z[e];
    return SG_OK;
}
int sg_gradient_penalty_fwd_cpu(const float* grad, long B, long M, float weight, float* norms, float* loss, void*) {
    CPU_CHECK(grad && norms && loss && B > 0 && M > 0);
    double acc = 0;
    for (long b = 0; b < B; ++b) {
        double s = 0;
        for (long e = 0; e < M; ++e) s += (double)grad[b * M + e] * grad[b * M + e];
        norms[b] = (float)sqrt(s);
        acc += ((double)norms[b] - 1.0) * ((double)norms[b] - 1.0);
    }
    loss[0] = (float)(acc / (double)B * (double)weight);
    return SG_OK;
}
int sg_gradient_penalty_bwd_cpu(const float* grad, const float* norms, const float* gloss, float* dgrad, long B, long M, float weight, void*) {
    CPU_CHECK(grad && norms && gloss && dgrad && B > 0 && M > 0);
    const float coef = (float)(2.0 * (double)weight / (double)B);
    for (long b = 0; b < B; ++b) {
        const float c = norms[b] > 0.f ? gloss[0] * coef * (norms[b] - 1.f) / norms[b] : 0.f;
        for (long e = 0; e < M; ++e) dgrad[b * M + e] = c * grad[b * M + e];
    }
    return SG_OK;
}
int sg_lerp_rows_cpu(const float* a, const float* b, const float* alpha, float* out, long B, long M, void*) {
    CPU_CHECK(a && b && alpha && out && B > 0 && M > 0);
    for (long r = 0; r < B; ++r) {
        const float al = alpha[r], be = 1.f - al;
        for (long e = 0; e < M; ++e) {
            const float t1 = al * a[r * M + e], t2 = be * b[r * M + e];
            out[r * M + e] = t1 + t2;
        }
    }
    return SG_OK;
}
int sg_fade_blend_cpu(const float* x, const float* half, float* out, long B, int C, long S, float fade, float hs, void*) {
    CPU_CHECK(half && out && B > 0 && C > 0 && S > 0);
    for (long b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (long e = 0; e < S; ++e) {
                float v = x ? fade * x[(b * C + c) * S + e] : 0.f;
                if (c == 0) v = v + hs * half[b * S + e];
                out[(b * C + c) * S + e] = v;
            }
    return SG_OK;
}
int sg_channel0_cpu(const float* g, float* out, long B, int C, long S, float scale, void*) {
    CPU_CHECK(g && out && B > 0 && C > 0 && S > 0);
    for (long b = 0; b < B; ++b)
        for (long e = 0; e < S; ++e) out[b * S + e] = scale * g[b * C * S + e];
    return SG_OK;
}
int sg_subsample2_cpu(const float* x, float* out, long B, int R, void*) {
    CPU_CHECK(x && out && B > 0 && R >= 2 && !(R & 1));
    const int h = R / 2;
    for (long b = 0; b < B; ++b)
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < h; ++j)
                for (int k = 0; k < h; ++k) out[((b * h + i) * h + j) * h + k] = x[((b * R + 2 * i) * R + 2 * j) * R + 2 * k];
    return SG_OK;
}
int sg_subsample2_adjoint_cpu(const float* g, float* out, long B, int R, void*) {
    CPU_CHECK(g && out && B > 0 && R >= 2 && !(R & 1));
    const int h = R / 2;
    memset(out, 0, sizeof(float) * B * R * R * R);
    for (long b = 0; b < B; ++b)
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < h; ++j)
                for (int k = 0; k < h; ++k) out[((b * R + 2 * i) * R + 2 * j) * R + 2 * k] = g[((b * h + i) * h + j) * h + k];
    return SG_OK;
}

// ---- PointNet family ------------------------------------------------------------------------------------------------------------
int sg_layernorm_fwd_cpu(const float* x, long ldx, const float* rowbias, long rows_per_shape, const float* gamma,
                         const float* beta, float* y, long ldy, float* mean, float* rstd, long R, int C, float eps, int act, void*) {
    CPU_CHECK(x && gamma && beta && y && mean && rstd && R > 0 && C > 0 && (act == ACT_NONE || act == ACT_RELU));
#pragma omp parallel for schedule(static)
    for (long r = 0; r < R; ++r) {
        const float* zb = rowbias ? rowbias + (r / rows_per_shape) * C : nullptr;
        double s = 0, s2 = 0;
        for (int c = 0; c < C; ++c) s += x[r * ldx + c] + (zb ? zb[c] : 0.f);
        const double mu = s / C;
        for (int c = 0; c < C; ++c) {
            const double d = x[r * ldx + c] + (zb ? zb[c] : 0.f) - mu;
            s2 += d * d;
        }
        const float rs = (float)(1.0 / sqrt(s2 / C + (double)eps));
        mean[r] = (float)mu;
        rstd[r] = rs;
        for (int c = 0; c < C; ++c) {
            const float v = gamma[c] * ((x[r * ldx + c] + (zb ? zb[c] : 0.f) - (float)mu) * rs) + beta[c];
            y[r * ldy + c] = act == ACT_RELU ? (v > 0.f ? v : 0.f) : v;
        }
    }
    return SG_OK;
}
int sg_layernorm_bwd_cpu(const float* x, long ldx, const float* rowbias, long rows_per_shape, const float* gamma, const float* y,
                         long ldy, const float* dy, long lddy, const float* mean, const float* rstd, float* dz, long lddz,
                         float* dgamma, float* dbeta, long R, int C, int act, void*, size_t, void*) {
    CPU_CHECK(x && gamma && dy && mean && rstd && dz && dgamma && dbeta && R > 0 && C > 0);
    std::vector<double> ag(C, 0.0), ab(C, 0.0);
    for (long r = 0; r < R; ++r) {
        const float* zb = rowbias ? rowbias + (r / rows_per_shape) * C : nullptr;
        const float mu = mean[r], rs = rstd[r];
        double s1 = 0, s2 = 0;
        std::vector<float> xh(C), gh(C);
        for (int c = 0; c < C; ++c) {
            float g = dy[r * lddy + c];
            if (act == ACT_RELU) g = y[r * ldy + c] > 0.f ? g : 0.f;
            xh[c] = (x[r * ldx + c] + (zb ? zb[c] : 0.f) - mu) * rs;
            gh[c] = g * gamma[c];
            ag[c] += (double)g * xh[c];
            ab[c] += g;
            s1 += gh[c];
            s2 += (double)gh[c] * xh[c];
        }
        const float m1 = (float)(s1 / C), m2 = (float)(s2 / C);
        for (int c = 0; c < C; ++c) dz[r * lddz + c] = rs * (gh[c] - m1 - xh[c] * m2);
    }
    for (int c = 0; c < C; ++c) {
        dgamma[c] = (float)ag[c];
        dbeta[c] = (float)ab[c];
    }
    return SG_OK;
}
int sg_segmax_fwd_cpu(const float* x, float* out, int* idx, long B, long P, int C, void*, size_t, void*) {
    CPU_CHECK(x && out && idx && B > 0 && P > 0 && C > 0);
    // torch.max semantics: first occurrence of the maximum; a NaN wins and the first NaN is reported
    for (long b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            float best = x[(b * P) * C + c];
            int arg = 0;
            for (long p = 1; p < P && best == best; ++p) {
                const float v = x[(b * P + p) * C + c];
                if (v != v || v > best) {
                    best = v;
                    arg = (int)p;
                }
            }
            out[b * C + c] = best;
            idx[b * C + c] = arg;
        }
    return SG_OK;
}
int sg_segmax_scatter_cpu(const float* dy, const int* idx, float* dx, long B, long P, int C, void*) {
    CPU_CHECK(dy && idx && dx && B > 0 && P > 0 && C > 0);
    memset(dx, 0, sizeof(float) * B * P * C);
    for (long b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) dx[(b * P + idx[b * C + c]) * C + c] = dy[b * C + c];
    return SG_OK;
}
int sg_scatter_rows_grouped_cpu(const float* g, const int64_t* rows, float* dx, long B, int C, int K, void*) {
    CPU_CHECK(g && rows && dx && B > 0 && C > 0 && C <= 1024 && K > 0);
    for (long b = 0; b < B; ++b)
        for (int c2 = 0; c2 < C; ++c2) {
            const int64_t mine = rows[b * C + c2];
            bool led = false;
            for (int e = 0; e < c2 && !led; ++e) led = rows[b * C + e] == mine;
            if (led) continue;
            for (int k = 0; k < K; ++k) {
                float s = g[(b * C + c2) * K + k];
                for (int e = c2 + 1; e < C; ++e)
                    if (rows[b * C + e] == mine) s += g[(b * C + e) * K + k];
                dx[mine * K + k] = s;
            }
        }
    return SG_OK;
}
int sg_rowdot_cpu(const float* h, const float* w, const float* bias, float* out, long B, int C, int K, void*) {
    CPU_CHECK(h && w && out && B > 0 && C > 0 && K > 0);
#pragma omp parallel for schedule(static)
    for (long r = 0; r < B * C; ++r) {
        const int c = (int)(r % C);
        double s = bias ? bias[c] : 0.0;
        for (int k = 0; k < K; ++k) s += (double)h[r * K + k] * w[(long)c * K + k];
        out[r] = (float)s;
    }
    return SG_OK;
}
int sg_rowscale_cpu(const float* g, const float* w, float* out, long B, int C, int K, void*) {
    CPU_CHECK(g && w && out && B > 0 && C > 0 && K > 0);
#pragma omp parallel for schedule(static)
    for (long r = 0; r < B * C; ++r)
        for (int k = 0; k < K; ++k) out[r * K + k] = g[r] * w[(long)(r % C) * K + k];
    return SG_OK;
}
int sg_rowouter_cpu(const float* g, const float* h, float* out, long B, int C, int K, void*) {
    CPU_CHECK(g && h && out && B > 0 && C > 0 && K > 0);
#pragma omp parallel for schedule(static)
    for (long e = 0; e < (long)C * K; ++e) {
        const long c = e / K, k = e % K;
        double s = 0;
        for (long b = 0; b < B; ++b) s += (double)g[b * C + c] * h[(b * C + c) * K + k];
        out[e] = (float)s;
    }
    return SG_OK;
}
int sg_segmax_gather_cpu(const float* x, const int* idx, float* out, long B, long P, int C, void*) {
    CPU_CHECK(x && idx && out && B > 0 && P > 0 && C > 0);
    for (long b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) out[b * C + c] = x[(b * P + idx[b * C + c]) * C + c];
    return SG_OK;
}
int sg_scatter_max_fwd_cpu(const float* x, const int64_t* batch, float* out, int* arg, long N, long B, int C, void*, size_t, void*) {
    CPU_CHECK(x && batch && out && arg && N > 0 && B > 0 && C > 0);
    for (long e = 0; e < B * C; ++e) {
        arg[e] = -1;
        out[e] = 0.f;
    }
    for (long i = 0; i < N; ++i) {
        const long b = batch[i];
        if (b < 0 || b >= B) continue;
        for (int c = 0; c < C; ++c)
            if (arg[b * C + c] < 0 || x[i * C + c] > out[b * C + c]) {
                out[b * C + c] = x[i * C + c];
                arg[b * C + c] = (int)i;
            }
    }
    return SG_OK;
}
int sg_scatter_max_scatter_cpu(const float* dy, const int* arg, float* dx, long N, long B, int C, void*) {
    CPU_CHECK(dy && arg && dx && N > 0 && B > 0 && C > 0);
    memset(dx, 0, sizeof(float) * N * C);
    for (long e = 0; e < B * C; ++e)
        if (arg[e] >= 0) dx[(long)arg[e] * C + e % C] = dy[e];
    return SG_OK;
}
int sg_scatter_max_gather_cpu(const float* x, const int* arg, float* out, long N, long B, int C, void*) {
    CPU_CHECK(x && arg && out && N > 0 && B > 0 && C > 0);
    for (long e = 0; e < B * C; ++e) out[e] = arg[e] >= 0 ? x[(long)arg[e] * C + e % C] : 0.f;
    return SG_OK;
}

}  // extern "C"

// ---- the areas that promise the bits of the HIP kernels: K12, sphere tracing, K13, K15 ---------------------------------------------
// Their per-element arithmetic is csrc/*_core.h, the files the HIP kernels include: one statement of every formula.  What is written
// here is the part the headers leave to each library: the loops, the lists and the summations.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/mesh_core.h"
#include "../csrc/raymarch_core.h"
#include "../csrc/pointcloud_core.h"
#include "../csrc/topology_core.h"
#include "../csrc/simplify_core.h"

extern "C" {

// ---- K12: marching cubes and surface sampling (csrc/mesh.hip) ------------------------------------------------------------------
// The same cells in the same order as the kernels: the corners of the (virtually padded) grid in row-major order, each owning the
// crossing edges at its minimum corner (axes 0, 1, 2) and, where it exists, the cube with that minimum corner.
int sg_mc_count_cpu(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, int64_t* vert_offsets,
                    int64_t* tri_offsets, void*, size_t, void*) {
    SgMcGrid m;
    long cells = 0;
    CPU_CHECK(grids && sg_mc_grid(m, S, R0, R1, R2, level, pad, pad_value, cells));
    CPU_CHECK(vert_offsets && tri_offsets);
    std::vector<int64_t> nv(S), nt(S);
#pragma omp parallel for schedule(dynamic)
    for (long s = 0; s < S; ++s) {
        const float* g = grids + s * (long)R0 * R1 * R2;
        int64_t v = 0, t = 0;
        float val[8];
        for (int a = 0; a < m.P0; ++a)
            for (int b = 0; b < m.P1; ++b)
                for (int c = 0; c < m.P2; ++c) {
                    sg_mc_corners(m, g, a, b, c, val);
                    const SgMcCell r = sg_mc_classify(m, val, a, b, c);
                    v += r.nv;
                    t += r.nt;
                }
        nv[s] = v;
        nt[s] = t;
    }
    vert_offsets[0] = tri_offsets[0] = 0;
    for (long s = 0; s < S; ++s) {
        vert_offsets[s + 1] = vert_offsets[s] + nv[s];
        tri_offsets[s + 1] = tri_offsets[s] + nt[s];
    }
    return SG_OK;
}

int sg_mc_emit_cpu(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, float sx, float sy,
                   float sz, float ox, float oy, float oz, const int64_t* vert_offsets, const int64_t* tri_offsets, float* vertices,
                   float* normals, int64_t* faces, long max_verts, long max_tris, void*, size_t, void*) {
    SgMcGrid m;
    long cells = 0;
    CPU_CHECK(grids && sg_mc_grid(m, S, R0, R1, R2, level, pad, pad_value, cells));
    CPU_CHECK(vert_offsets && tri_offsets && max_verts >= 0 && max_tris >= 0);
    CPU_CHECK((max_verts == 0 || (vertices && normals)) && (max_tris == 0 || faces));
    CPU_CHECK(vert_offsets[S] <= max_verts && tri_offsets[S] <= max_tris);
    const float sp[3] = {sx, sy, sz}, org[3] = {ox, oy, oz};
#pragma omp parallel for schedule(dynamic)
    for (long s = 0; s < S; ++s) {
        const float* g = grids + s * (long)R0 * R1 * R2;
        std::vector<int> first(cells), owned(cells);      // per cell: first vertex (local to the shape), crossing mask
        long vo = 0, to = 0;
        float v[8];
        long cell = 0;
        for (int a = 0; a < m.P0; ++a)
            for (int b = 0; b < m.P1; ++b)
                for (int c = 0; c < m.P2; ++c, ++cell) {
                    sg_mc_corners(m, g, a, b, c, v);
                    const int mask = sg_mc_classify(m, v, a, b, c).mask;
                    first[cell] = (int)vo;
                    owned[cell] = mask;
                    if (!mask) continue;
                    float g0[3];
                    for (int k = 0; k < 3; ++k) g0[k] = sg_mc_grad(m, g, a, b, c, k, sp[k]);
                    for (int axis = 0; axis < 3; ++axis) {
                        if (!((mask >> axis) & 1)) continue;
                        const long out = vert_offsets[s] + vo;
                        sg_mc_vertex(m, g, sp, org, a, b, c, v, g0, axis, vertices + out * 3, normals + out * 3);
                        ++vo;
                    }
                }
        const long plane = (long)m.P1 * m.P2;
        cell = 0;
        for (int a = 0; a < m.P0; ++a)
            for (int b = 0; b < m.P1; ++b)
                for (int c = 0; c < m.P2; ++c, ++cell) {
                    sg_mc_corners(m, g, a, b, c, v);
                    const SgMcCell r = sg_mc_classify(m, v, a, b, c);
                    for (int j = 0; j < r.nt; ++j) {
                        const long f = tri_offsets[s] + to + j;
                        for (int k = 0; k < 3; ++k) {
                            int oa, ob, oc;
                            const int axis = sg_mc_edge_owner(sg_mc_tri_edges[r.cube][3 * j + k], oa, ob, oc);
                            const long owner = (long)(a + oa) * plane + (long)(b + ob) * m.P2 + (c + oc);
                            faces[f * 3 + k] = first[owner] + sg_mc_rank(owned[owner], axis);
                        }
                    }
                    to += r.nt;
                }
    }
    return SG_OK;
}

int sg_mesh_sample_cpu(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S,
                       long F, const float* uniforms, long P, float* out, int* empty, void*, size_t, void*) {
    CPU_CHECK(vert_offsets && tri_offsets && uniforms && out && empty && S > 0 && P > 0 && F >= 0);
    CPU_CHECK(F == 0 || (vertices && faces));
#pragma omp parallel for schedule(dynamic)
    for (long s = 0; s < S; ++s) {
        const long f0 = tri_offsets[s], f1 = tri_offsets[s + 1], vb = vert_offsets[s];
        empty[s] = f1 > f0 ? 0 : 1;
        if (f1 <= f0) {
            memset(out + s * P * 3, 0, sizeof(float) * P * 3);
            continue;
        }
        // cumulative doubled areas in double, added in triangle order
        std::vector<double> cdf(f1 - f0);
        double run = 0.0;
        for (long f = f0; f < f1; ++f) {
            run += sg_mesh_area2(vertices + (vb + faces[f * 3]) * 3, vertices + (vb + faces[f * 3 + 1]) * 3, vertices + (vb + faces[f * 3 + 2]) * 3);
            cdf[f - f0] = run;
        }
        for (long q = 0; q < P; ++q) {
            const long i = s * P + q;
            const float u0 = uniforms[i * 3], u1 = uniforms[i * 3 + 1], u2 = uniforms[i * 3 + 2];
            const double x = (double)u0 * cdf.back();
            const long k = std::min((long)(std::lower_bound(cdf.begin(), cdf.end(), x) - cdf.begin()), f1 - f0 - 1);
            const long f = f0 + k;
            sg_mesh_point(vertices + (vb + faces[f * 3]) * 3, vertices + (vb + faces[f * 3 + 1]) * 3, vertices + (vb + faces[f * 3 + 2]) * 3, u1, u2,
                          out + i * 3);
        }
    }
    return SG_OK;
}

// ---- K12b: mesh topology (csrc/topology.hip) -------------------------------------------------------------------------------------
// The same partition, numbering, keys, counts and tile sums as the kernels, walked in order on one thread (the tile sums per component
// in parallel): a sequential union-find whose roots are the lowest vertices, the header's tree per tile.
static bool topo_sizes(long S, long V, long F) { return S >= 1 && S < 2147483647L && V >= 0 && F >= 0 && V <= 2147483647L && F <= 2147483647L; }

static bool topo_corners(const int64_t* faces, const int64_t* vo, const int64_t* to, long S, long V, long f, long& s, long& a, long& b, long& c) {
    s = sg_topo_shape_of(to, S, f);
    return sg_topo_triangle(faces + f * 3, vo[s], vo[s + 1] - vo[s], V, a, b, c);
}

static long topo_component_of(const int64_t* vo, long S, long v, const int* vertex_component, const int64_t* comp_offsets, long C) {
    const int label = vertex_component[v];
    if (label < 0) return -1;
    const long c = comp_offsets[sg_topo_shape_of(vo, S, v)] + label;
    return c < C ? c : -1;
}

static int topo_find(std::vector<int>& parent, int x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

// out[t] = the position of the first element of shape t among the set flags (t = S: their number); excl: the positions
static void topo_scan(const std::vector<int>& flag, long n, int* excl, const int64_t* offsets, long S, int64_t* out) {
    int run = 0;
    for (long i = 0; i < n; ++i) {
        excl[i] = run;
        run += flag[i];
    }
    for (long t = 0; t <= S; ++t) {
        const long o = offsets[t];
        out[t] = t == S || o >= n ? run : (o < 0 ? 0 : excl[o]);
    }
}

int sg_topo_label_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                      int* vertex_component, int64_t* comp_offsets, void*, size_t, void*) {
    CPU_CHECK(topo_sizes(S, V, F));
    CPU_CHECK(vert_offsets && tri_offsets && comp_offsets && (V == 0 || vertex_component) && (F == 0 || faces));
    std::vector<int> parent(V), named(V, 0), is_root(V), excl(V);
    for (long v = 0; v < V; ++v) parent[v] = (int)v;
    for (long f = 0; f < F; ++f) {
        long s, c[3];
        if (!topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, c[0], c[1], c[2])) continue;
        for (int k = 0; k < 3; ++k) named[c[k]] = 1;
        for (int k = 0; k < 2; ++k) {
            const int ra = topo_find(parent, (int)c[k]), rb = topo_find(parent, (int)c[k + 1]);
            if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
        }
    }
    for (long v = 0; v < V; ++v) is_root[v] = topo_find(parent, (int)v) == (int)v && named[v];
    topo_scan(is_root, V, excl.data(), vert_offsets, S, comp_offsets);
    for (long v = 0; v < V; ++v)
        vertex_component[v] = named[v] ? (int)((long)excl[topo_find(parent, (int)v)] - comp_offsets[sg_topo_shape_of(vert_offsets, S, v)]) : -1;
    return SG_OK;
}

int sg_topo_keys_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                     const int* vertex_component, const int64_t* comp_offsets, long C, int* tri_keys, int64_t* edge_keys, void*) {
    CPU_CHECK(topo_sizes(S, V, F) && C >= 0 && C <= V);
    CPU_CHECK(vert_offsets && tri_offsets && comp_offsets && (V == 0 || vertex_component) && (F == 0 || (faces && tri_keys && edge_keys)));
    for (long f = 0; f < F; ++f) {
        long s, a, b, c, comp = -1;
        if (topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c)) comp = topo_component_of(vert_offsets, S, a, vertex_component, comp_offsets, C);
        tri_keys[f] = comp < 0 ? SG_TOPO_NO_COMPONENT : (int)comp;
        edge_keys[3 * f] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(a, b);
        edge_keys[3 * f + 1] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(b, c);
        edge_keys[3 * f + 2] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(c, a);
    }
    return SG_OK;
}

int sg_topo_stats_cpu(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S,
                      long V, long F, const int* vertex_component, const int64_t* comp_offsets, long C, const int64_t* tri_order,
                      const int64_t* seg_offsets, const int64_t* tile_offsets, const int64_t* edge_sorted, int* n_vertices,
                      int* n_triangles, int* n_edges, int* n_open, double* area, double* volume, void*, size_t, void*) {
    CPU_CHECK(topo_sizes(S, V, F) && C >= 0 && C <= V);
    CPU_CHECK(vert_offsets && tri_offsets && comp_offsets && seg_offsets && tile_offsets);
    CPU_CHECK((V == 0 || (vertices && vertex_component)) && (F == 0 || (faces && tri_order && edge_sorted)));
    CPU_CHECK(C == 0 || (n_vertices && n_triangles && n_edges && n_open && area && volume));
    for (long c = 0; c < C; ++c) n_vertices[c] = n_edges[c] = n_open[c] = 0;
    if (C == 0) return SG_OK;
    for (long v = 0; v < V; ++v) {
        const long comp = topo_component_of(vert_offsets, S, v, vertex_component, comp_offsets, C);
        if (comp >= 0) ++n_vertices[comp];
    }
    for (long i = 0; i < 3 * F;) {
        const int64_t key = edge_sorted[i];
        if (key == SG_TOPO_NO_EDGE || key < 0) {
            ++i;
            continue;
        }
        long forward = 0, backward = 0, j = i;
        for (; j < 3 * F && sg_topo_same_edge(edge_sorted[j], key); ++j) (edge_sorted[j] & 1 ? backward : forward) += 1;
        const long low = sg_topo_edge_low(key);
        const long comp = low < V ? topo_component_of(vert_offsets, S, low, vertex_component, comp_offsets, C) : -1;
        if (comp >= 0) {
            ++n_edges[comp];
            if (!(forward == 1 && backward == 1)) ++n_open[comp];
        }
        i = j;
    }
#pragma omp parallel for schedule(dynamic, 16)
    for (long c = 0; c < C; ++c) {
        const long i0 = seg_offsets[c], i1 = seg_offsets[c + 1];
        double sa = 0.0, sv = 0.0;
        for (long t = 0; t < tile_offsets[c + 1] - tile_offsets[c]; ++t) {
            double ta[SG_TOPO_TILE], tv[SG_TOPO_TILE];
            for (int l = 0; l < SG_TOPO_TILE; ++l) {
                const long i = i0 + t * SG_TOPO_TILE + l;
                ta[l] = tv[l] = 0.0;
                if (i >= i1 || i < 0 || i >= F) continue;
                const long f = tri_order[i];
                long s, a, b, cc;
                if (f >= 0 && f < F && topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, cc))
                    sg_topo_terms(vertices + a * 3, vertices + b * 3, vertices + cc * 3, ta[l], tv[l]);
            }
            for (int g = 0; g < SG_TOPO_TILE; g += 64)
                for (int off = 32; off > 0; off >>= 1)
                    for (int l = 0; l < off; ++l) {
                        ta[g + l] += ta[g + l + off];
                        tv[g + l] += tv[g + l + off];
                    }
            sa += ((ta[0] + ta[64]) + ta[128]) + ta[192];
            sv += ((tv[0] + tv[64]) + tv[128]) + tv[192];
        }
        n_triangles[c] = (int)(i1 - i0);
        area[c] = sa;
        volume[c] = sv;
    }
    return SG_OK;
}

int sg_topo_keep_count_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                           const int* vertex_component, const int64_t* comp_offsets, long C, const uint8_t* keep,
                           int64_t* new_vert_offsets, int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes, void*) {
    CPU_CHECK(topo_sizes(S, V, F) && C >= 0 && C <= V);
    CPU_CHECK(vert_offsets && tri_offsets && comp_offsets && new_vert_offsets && new_tri_offsets && workspace);
    CPU_CHECK((V == 0 || vertex_component) && (F == 0 || faces) && (C == 0 || keep));
    CPU_CHECK(workspace_bytes >= (size_t)(2 * V + 2 * F) * sizeof(int));
    int *kept_v = (int*)workspace, *pos_v = kept_v + V, *kept_t = pos_v + V, *pos_t = kept_t + F;
    std::vector<int> kv(V), kt(F);
    for (long v = 0; v < V; ++v) {
        const long comp = topo_component_of(vert_offsets, S, v, vertex_component, comp_offsets, C);
        kept_v[v] = kv[v] = comp >= 0 && keep[comp] ? 1 : 0;
    }
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        kept_t[f] = kt[f] = topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c) && kv[a] ? 1 : 0;
    }
    topo_scan(kv, V, pos_v, vert_offsets, S, new_vert_offsets);
    topo_scan(kt, F, pos_t, tri_offsets, S, new_tri_offsets);
    return SG_OK;
}

int sg_topo_keep_emit_cpu(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                          const int64_t* tri_offsets, long S, long V, long F, const int64_t* new_vert_offsets, float* out_vertices,
                          float* out_normals, int64_t* out_faces, long max_verts, long max_tris, void* workspace,
                          size_t workspace_bytes, void*) {
    CPU_CHECK(topo_sizes(S, V, F) && max_verts >= 0 && max_tris >= 0);
    CPU_CHECK(vert_offsets && tri_offsets && new_vert_offsets && workspace);
    CPU_CHECK((V == 0 || (vertices && normals)) && (F == 0 || faces));
    CPU_CHECK((max_verts == 0 || (out_vertices && out_normals)) && (max_tris == 0 || out_faces));
    CPU_CHECK(workspace_bytes >= (size_t)(2 * V + 2 * F) * sizeof(int));
    const int *kept_v = (const int*)workspace, *pos_v = kept_v + V, *kept_t = pos_v + V, *pos_t = kept_t + F;
    for (long v = 0; v < V; ++v) {
        if (!kept_v[v] || pos_v[v] >= max_verts) continue;
        memcpy(out_vertices + (long)pos_v[v] * 3, vertices + v * 3, 3 * sizeof(float));
        memcpy(out_normals + (long)pos_v[v] * 3, normals + v * 3, 3 * sizeof(float));
    }
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        if (!kept_t[f] || pos_t[f] >= max_tris || !topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c)) continue;
        const long base = new_vert_offsets[s], o = pos_t[f];
        out_faces[o * 3] = pos_v[a] - base;
        out_faces[o * 3 + 1] = pos_v[b] - base;
        out_faces[o * 3 + 2] = pos_v[c] - base;
    }
    return SG_OK;
}

// ---- K12c: mesh simplification (csrc/simplify.hip) -------------------------------------------------------------------------------
// The same keys, cluster numbers, corner records, sums (the header's tiles of 64) and compaction as the kernels, walked in order; the
// clusters are placed in parallel.
static bool simp_sizes(long S, long V, long F) {
    return S >= 1 && S < SG_SIMPLIFY_MAX_SHAPES && V >= 0 && F >= 0 && V <= 2147483647L && F <= 2147483647L;
}

int sg_simplify_bounds_cpu(const float* vertices, const int64_t* vert_offsets, long S, long V, float* lo, float* hi, void*) {
    CPU_CHECK(simp_sizes(S, V, 0));
    CPU_CHECK(vert_offsets && lo && hi && (V == 0 || vertices));
    for (long s = 0; s < S; ++s) {
        const long v0 = std::max<long>(vert_offsets[s], 0), v1 = std::min<long>(vert_offsets[s + 1], V);
        for (int k = 0; k < 3; ++k) {
            int mn = sg_float_key(3.4028234663852886e38f), mx = sg_float_key(-3.4028234663852886e38f);
            for (long v = v0; v < v1; ++v) {
                const float x = vertices[v * 3 + k];
                if (!(fabsf(x) <= 3.4028234663852886e38f)) continue;
                mn = std::min(mn, sg_float_key(x));
                mx = std::max(mx, sg_float_key(x));
            }
            lo[s * 3 + k] = mn <= mx ? sg_key_float(mn) : 0.0f;
            hi[s * 3 + k] = mn <= mx ? sg_key_float(mx) : 0.0f;
        }
    }
    return SG_OK;
}

int sg_simplify_keys_cpu(const float* vertices, const int64_t* vert_offsets, long S, long V, const float* origin, const float* cell,
                         const int* cells, int64_t* keys, void*) {
    CPU_CHECK(simp_sizes(S, V, 0));
    CPU_CHECK(vert_offsets && origin && cell && cells && (V == 0 || (vertices && keys)));
    for (long v = 0; v < V; ++v) {
        const long s = sg_topo_shape_of(vert_offsets, S, v);
        keys[v] = sg_simplify_key(s, vertices + v * 3, origin + s * 3, cell[s * 2 + 1], cells[s]);
    }
    return SG_OK;
}

int sg_simplify_count_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                          const int64_t* keys, int* counts, void*) {
    CPU_CHECK(simp_sizes(S, V, F));
    CPU_CHECK(vert_offsets && tri_offsets && counts && (V == 0 || keys) && (F == 0 || faces));
    for (long s = 0; s < S; ++s) counts[s] = 0;
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        if (!topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c)) continue;
        if (keys[a] != keys[b] && keys[b] != keys[c] && keys[a] != keys[c]) ++counts[s];
    }
    return SG_OK;
}

int sg_simplify_clusters_cpu(const int64_t* sorted_keys, const int64_t* order, const int64_t* vert_offsets, long S, long V,
                             int* sorted_cluster, int* vertex_cluster, int64_t* cluster_offsets, void*, size_t, void*) {
    CPU_CHECK(simp_sizes(S, V, 0));
    CPU_CHECK(vert_offsets && cluster_offsets && (V == 0 || (sorted_keys && order && sorted_cluster && vertex_cluster)));
    std::vector<int> head(V), excl(V);
    for (long i = 0; i < V; ++i) head[i] = i == 0 || sorted_keys[i] != sorted_keys[i - 1];
    topo_scan(head, V, excl.data(), vert_offsets, S, cluster_offsets);
    for (long i = 0; i < V; ++i) {
        sorted_cluster[i] = excl[i] + head[i] - 1;
        if (order[i] >= 0 && order[i] < V) vertex_cluster[order[i]] = sorted_cluster[i];
    }
    return SG_OK;
}

int sg_simplify_corners_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                            const int* vertex_cluster, int64_t* corner_keys, void*) {
    CPU_CHECK(simp_sizes(S, V, F));
    CPU_CHECK(vert_offsets && tri_offsets && (V == 0 || vertex_cluster) && (F == 0 || (faces && corner_keys)));
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        const bool counts = topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c);
        sg_simplify_corner_keys(counts, counts ? vertex_cluster[a] : 0, counts ? vertex_cluster[b] : 0, counts ? vertex_cluster[c] : 0, f,
                                corner_keys + 3 * f);
    }
    return SG_OK;
}

// the header's tree over one tile: s[l] += s[l + off] for off = 32 .. 1; returns s[0]
static double simp_tile(double* s) {
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) s[l] += s[l + off];
    return s[0];
}

int sg_simplify_place_cpu(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                          const int64_t* tri_offsets, long S, long V, long F, const int64_t* sorted_keys, const int64_t* order,
                          const int* sorted_cluster, const int64_t* corner_sorted, long C, const float* origin, const float* cell,
                          int placement, float* cluster_vertices, float* cluster_normals, void*) {
    CPU_CHECK(simp_sizes(S, V, F) && C >= 0 && C <= V);
    CPU_CHECK(placement == SG_SIMPLIFY_QUADRIC || placement == SG_SIMPLIFY_MEAN);
    CPU_CHECK(vert_offsets && tri_offsets && origin && cell);
    CPU_CHECK(V == 0 || (vertices && normals && sorted_keys && order && sorted_cluster));
    CPU_CHECK(F == 0 || placement == SG_SIMPLIFY_MEAN || (faces && corner_sorted));
    CPU_CHECK(C == 0 || (cluster_vertices && cluster_normals));
#pragma omp parallel for schedule(dynamic, 64)
    for (long c = 0; c < C; ++c) {
        const long v0 = std::lower_bound(sorted_cluster, sorted_cluster + V, (int)c) - sorted_cluster;
        const long v1 = c + 1 > 2147483647L ? V : std::lower_bound(sorted_cluster, sorted_cluster + V, (int)(c + 1)) - sorted_cluster;
        if (v0 >= v1) {
            for (int k = 0; k < 3; ++k) cluster_vertices[c * 3 + k] = cluster_normals[c * 3 + k] = 0.0f;
            continue;
        }
        const int64_t key = sorted_keys[v0];
        const long s = std::min(std::max(sg_simplify_key_shape(key), 0L), S - 1);
        const float h = cell[s * 2];
        double p0[3];
        sg_simplify_centre(key, origin + s * 3, h, p0);
        double vsum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tile[9][SG_SIMPLIFY_TILE];
        for (long base = v0; base < v1; base += SG_SIMPLIFY_TILE) {
            for (int l = 0; l < SG_SIMPLIFY_TILE; ++l) {
                const long i = base + l, v = i < v1 ? order[i] : -1;
                for (int k = 0; k < 3; ++k) {
                    tile[k][l] = v >= 0 && v < V ? (double)vertices[v * 3 + k] : 0.0;
                    tile[3 + k][l] = v >= 0 && v < V ? (double)normals[v * 3 + k] : 0.0;
                }
            }
            for (int k = 0; k < 6; ++k) vsum[k] += simp_tile(tile[k]);
        }
        double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (placement == SG_SIMPLIFY_QUADRIC) {
            const int64_t* end = corner_sorted + 3 * F;
            const long c0 = std::lower_bound(corner_sorted, end, (int64_t)c << 31) - corner_sorted;
            const long c1 = std::lower_bound(corner_sorted, end, (int64_t)(c + 1) << 31) - corner_sorted;
            for (long base = c0; base < c1; base += SG_SIMPLIFY_TILE) {
                for (int l = 0; l < SG_SIMPLIFY_TILE; ++l) {
                    double x[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    const long i = base + l;
                    if (i < c1) {
                        const long f = sg_simplify_corner_triangle(corner_sorted[i]);
                        long ts, a, b, cc;
                        if (f < F && topo_corners(faces, vert_offsets, tri_offsets, S, V, f, ts, a, b, cc))
                            sg_simplify_quadric(vertices + a * 3, vertices + b * 3, vertices + cc * 3, p0, x);
                    }
                    for (int k = 0; k < 9; ++k) tile[k][l] = x[k];
                }
                for (int k = 0; k < 9; ++k) q[k] += simp_tile(tile[k]);
            }
        }
        const double count = (double)(v1 - v0);
        const double mean[3] = {vsum[0] / count, vsum[1] / count, vsum[2] / count};
        sg_simplify_place(q, mean, p0, h, placement, cluster_vertices + c * 3);
        sg_simplify_normal(vsum + 3, cluster_normals + c * 3);
    }
    return SG_OK;
}

int sg_simplify_faces_count_cpu(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                                const int* vertex_cluster, const int64_t* cluster_offsets, long C, int64_t* new_vert_offsets,
                                int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes, void*) {
    CPU_CHECK(simp_sizes(S, V, F) && C >= 0 && C <= V);
    CPU_CHECK(vert_offsets && tri_offsets && cluster_offsets && new_vert_offsets && new_tri_offsets && workspace);
    CPU_CHECK((V == 0 || vertex_cluster) && (F == 0 || faces));
    CPU_CHECK(workspace_bytes >= (size_t)(2 * C + 2 * F) * sizeof(int));
    int *named = (int*)workspace, *pos_c = named + C, *kept = pos_c + C, *pos_t = kept + F;
    std::vector<int> nm(C, 0), kt(F, 0);
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        if (!topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c)) continue;
        const long ca = vertex_cluster[a], cb = vertex_cluster[b], cc = vertex_cluster[c];
        if (ca != cb && cb != cc && ca != cc && ca >= 0 && cb >= 0 && cc >= 0 && ca < C && cb < C && cc < C) kt[f] = nm[ca] = nm[cb] = nm[cc] = 1;
    }
    for (long c = 0; c < C; ++c) named[c] = nm[c];
    for (long f = 0; f < F; ++f) kept[f] = kt[f];
    topo_scan(nm, C, pos_c, cluster_offsets, S, new_vert_offsets);
    topo_scan(kt, F, pos_t, tri_offsets, S, new_tri_offsets);
    return SG_OK;
}

int sg_simplify_faces_emit_cpu(const float* cluster_vertices, const float* cluster_normals, const int64_t* faces,
                               const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                               const int* vertex_cluster, long C, const int64_t* new_vert_offsets, float* out_vertices,
                               float* out_normals, int64_t* out_faces, long max_verts, long max_tris, void* workspace,
                               size_t workspace_bytes, void*) {
    CPU_CHECK(simp_sizes(S, V, F) && C >= 0 && C <= V && max_verts >= 0 && max_tris >= 0);
    CPU_CHECK(vert_offsets && tri_offsets && new_vert_offsets && workspace);
    CPU_CHECK((C == 0 || (cluster_vertices && cluster_normals)) && (V == 0 || vertex_cluster) && (F == 0 || faces));
    CPU_CHECK((max_verts == 0 || (out_vertices && out_normals)) && (max_tris == 0 || out_faces));
    CPU_CHECK(workspace_bytes >= (size_t)(2 * C + 2 * F) * sizeof(int));
    const int *named = (const int*)workspace, *pos_c = named + C, *kept = pos_c + C, *pos_t = kept + F;
    for (long c = 0; c < C; ++c) {
        if (!named[c] || pos_c[c] >= max_verts) continue;
        memcpy(out_vertices + (long)pos_c[c] * 3, cluster_vertices + c * 3, 3 * sizeof(float));
        memcpy(out_normals + (long)pos_c[c] * 3, cluster_normals + c * 3, 3 * sizeof(float));
    }
    for (long f = 0; f < F; ++f) {
        long s, a, b, c;
        if (!kept[f] || pos_t[f] >= max_tris || !topo_corners(faces, vert_offsets, tri_offsets, S, V, f, s, a, b, c)) continue;
        const long base = new_vert_offsets[s], o = pos_t[f];
        out_faces[o * 3] = pos_c[vertex_cluster[a]] - base;
        out_faces[o * 3 + 1] = pos_c[vertex_cluster[b]] - base;
        out_faces[o * 3 + 2] = pos_c[vertex_cluster[c]] - base;
    }
    return SG_OK;
}

// ---- sphere tracing (header: sg_raymarch_*; rendering/raymarching.py:render_image, get_shadows) ------------------------------
// The same lists, counts and segments as the HIP library; a step appends the survivors in list order (the HIP kernel in any
// order: the sets are the same).
// pre-activation of the last layer for one point, per-shape mode (packed of sg_sdfnet_pack_shape_bias_cpu, kin_used = 3)
static float rm_sdf_pre(const CpuSdf& v, const float* x, const float* zb1, const float* zb5) {
    float h[7][256];
    return sdf_shape_point_fwd(v, x, zb1, zb5, h);
}

int sg_raymarch_rays_cpu(const double* camera, int width, long nshapes, double radius, float* dir, float* pos, unsigned char* status,
                         int* active, int* counts, void*) {
    CPU_CHECK(camera && dir && pos && status && active && counts && width > 0 && nshapes > 0 && radius > 0.0);
    const long M = (long)width * width;
    CPU_CHECK(nshapes * M < (1L << 31));
    // (through a volatile: g++ 11 -O3's SLP vectoriser otherwise carries the double x and y of the camera past this rounding into
    // the start positions, 3e-8 off the float32 camera position that the header and the HIP kernel start from)
    const volatile float cfv[3] = {(float)camera[0], (float)camera[1], (float)camera[2]};
    const float cf[3] = {cfv[0], cfv[1], cfv[2]};
    const double cc =(camera[0] * camera[0] + camera[1] * camera[1] + camera[2] * camera[2]) - radius * radius;
    for (long pix = 0; pix < M; ++pix) {
        float p[3] = {cf[0], cf[1], cf[2]};
        const bool inside = sg_rm_camera_ray(camera, cc, width, pix, dir + pix * 3, p);
        for (long s = 0; s < nshapes; ++s) {
            const long r = s * M + pix;
            for (int c = 0; c < 3; ++c) pos[r * 3 + c] = p[c];
            status[r] = 0;
            if (inside) active[s * M + counts[s]++] = (int)r;
        }
    }
    return SG_OK;
}

int sg_raymarch_steps_cpu(const float* packed, const float* zb1, const float* zb5, float* pos, const float* dir, long dir_period,
                          unsigned char* status, int* active, long nrays, int* counts, const int64_t* seg_off, long nseg, long nshapes,
                          long max_rays, long first_iter, int steps, float clampv, float threshold, float sdf_offset, float radius0,
                          float radius1, int shadow, unsigned long long* evals, void*) {
    CPU_CHECK(packed && zb1 && zb5 && pos && dir && status && active && counts && seg_off && steps >= 0 && first_iter >= 0);
    CPU_CHECK(nseg > 0 && nseg <= 256 && nshapes > 0 && nseg % nshapes == 0 && nrays > 0 && nrays < (1L << 31));
    CPU_CHECK(max_rays >= 0 && max_rays <= nrays);
    if (max_rays == 0) return SG_OK;
    const CpuSdf v = sdf_view(packed, 3);
    std::vector<int> ray, seg;
    std::vector<float> sdf;
    for (int it = 0; it < steps; ++it) {
        const long iter = first_iter + it;
        const int* cr = counts + (iter % 3) * nseg;
        int* cw = counts + ((iter + 1) % 3) * nseg;
        const int* cur = active + (iter & 1) * nrays;
        int* next = active + ((iter + 1) & 1) * nrays;
        ray.clear();
        seg.clear();
        for (long s = 0; s < nseg; ++s) {
            const int c = cr[s];
            if (iter > 0 && c < 2) {
                if (c == 1) status[cur[seg_off[s]]] = 1;   // fewer than 2 left: the rest is a hit
                continue;
            }
            for (int k = 0; k < c; ++k) {
                ray.push_back(cur[seg_off[s] + k]);
                seg.push_back((int)s);
            }
        }
        for (long s = 0; s < nseg; ++s) counts[((iter + 2) % 3) * nseg + s] = 0;
        const long n = (long)ray.size();
        if (evals) *evals += (unsigned long long)n;
        sdf.resize(n);
#pragma omp parallel for schedule(dynamic, 16)
        for (long i = 0; i < n; ++i) {
            const long sh = seg[i] % nshapes;
            float s = tanhf(rm_sdf_pre(v, pos + (long)ray[i] * 3, zb1 + sh * 256, zb5 + sh * 256)) + sdf_offset;
            sdf[i] = std::min(std::max(s, -clampv), clampv);
        }
        for (long i = 0; i < n; ++i) {
            const long r = ray[i];
            const long di = dir_period > 0 ? r % dir_period : r;
            sg_rm_move(pos + r * 3, dir + di * 3, sdf[i]);
            if (sg_rm_hit(sdf[i], threshold)) {
                status[r] = 1;
                continue;
            }
            if (sg_rm_left(pos + r * 3, seg[i] < nshapes ? radius0 : radius1, shadow)) continue;
            next[seg_off[seg[i]] + cw[seg[i]]++] = (int)r;
        }
    }
    return SG_OK;
}

int sg_raymarch_finish_cpu(unsigned char* status, const int* active, long nrays, const int* counts, const int64_t* seg_off, long nseg,
                           long iter, void*) {
    CPU_CHECK(status && active && counts && seg_off && nseg > 0 && nseg <= 256 && iter >= 0 && nrays > 0);
    const int* cur = active + (iter & 1) * nrays;
    for (long s = 0; s < nseg; ++s)
        for (int k = 0; k < counts[(iter % 3) * nseg + s]; ++k) status[cur[seg_off[s] + k]] = 1;
    return SG_OK;
}

int sg_raymarch_classify_cpu(unsigned char* status, const float* pos, const float* dir, long M, long nshapes, int use_cutoff,
                             float vertical_cutoff, float* ground, int64_t* hit_off, int64_t* gnd_off, void*, size_t, void*) {
    CPU_CHECK(status && pos && dir && ground && hit_off && gnd_off && M > 0 && nshapes > 0 && 2 * nshapes <= 256);
    hit_off[0] = gnd_off[0] = 0;
    for (long s = 0; s < nshapes; ++s) {
        long h = 0;
        float g = INFINITY;
        for (long pix = 0; pix < M; ++pix) {
            const long r = s * M + pix;
            if (!status[r]) continue;
            const float y = pos[r * 3 + 1];
            if (use_cutoff && (y > vertical_cutoff || y < -vertical_cutoff)) {
                status[r] = 0;
                continue;
            }
            ++h;
            g = std::min(g, y);
        }
        ground[s] = g;
        hit_off[s + 1] = hit_off[s] + h;
        long n = 0;
        float q[3];
        if (h > 0)
            for (long pix = 0; pix < M; ++pix) n += sg_rm_ground_point(status[s * M + pix], pos + (s * M + pix) * 3, dir + pix * 3, g, q) ? 1 : 0;
        gnd_off[s + 1] = gnd_off[s] + n;
    }
    return SG_OK;
}

int sg_raymarch_emit_cpu(const unsigned char* status, const float* pos, const float* dir, long M, long nshapes, const float* ground,
                         const int64_t* hit_off, const int64_t* gnd_off, const double* light, float* hit_pos, int* hit_sid, int* slot,
                         float* shadow_pos, float* shadow_dir, int* shadow_active, int* shadow_counts, int64_t* shadow_seg,
                         const void*, size_t, void*) {
    CPU_CHECK(status && pos && dir && ground && hit_off && gnd_off && light && slot && shadow_counts && shadow_seg);
    CPU_CHECK(M > 0 && nshapes > 0 && 2 * nshapes <= 256);
    const long S = nshapes, H = hit_off[S];
    long h = 0, g = 0;
    for (long s = 0; s < S; ++s) {
        for (long pix = 0; pix < M; ++pix) {
            const long r = s * M + pix;
            float q[3];
            if (status[r]) {
                for (int c = 0; c < 3; ++c) q[c] = hit_pos[h * 3 + c] = pos[r * 3 + c];
                hit_sid[h] = (int)s;
                slot[r] = (int)h;
                sg_rm_shadow_ray(light, q, shadow_dir + h * 3, shadow_pos + h * 3);
                shadow_active[h] = (int)h;
                ++h;
            } else if (hit_off[s + 1] > hit_off[s] && sg_rm_ground_point(status[r], pos + r * 3, dir + pix * 3, ground[s], q)) {
                slot[r] = -2 - (int)g;
                sg_rm_shadow_ray(light, q, shadow_dir + (H + g) * 3, shadow_pos + (H + g) * 3);
                shadow_active[H + g] = (int)(H + g);
                ++g;
            } else {
                slot[r] = -1;
            }
        }
    }
    for (long j = 0; j <= 2 * S; ++j) shadow_seg[j] = j <= S ? hit_off[j] : H + gnd_off[j - S];
    for (long j = 0; j < 2 * S; ++j) {
        shadow_counts[j] = (int)(shadow_seg[j + 1] - shadow_seg[j]);
        shadow_counts[2 * S + j] = shadow_counts[4 * S + j] = 0;
    }
    return SG_OK;
}

int sg_raymarch_shade_cpu(const int* slot, const float* hit_pos, const float* grad, const unsigned char* shadow, const float* dir, long M,
                          long nshapes, long nhits, const double* light, const double* color, unsigned char* image, void*) {
    CPU_CHECK(slot && dir && light && color && image && M > 0 && nshapes > 0 && nhits >= 0);
    CPU_CHECK(nhits == 0 || (hit_pos && grad && shadow));
#pragma omp parallel for schedule(static)
    for (long r = 0; r < nshapes * M; ++r) {
        sg_rm_shade(slot[r], dir + (r % M) * 3, hit_pos, grad, shadow, nhits, light, color, image + r * 3);
    }
    return SG_OK;
}

// ---- K13: point-cloud evaluation (include/shapegan_hip.h) -------------------------------------------------------------------
static inline float cd_pair(const float* a, const float* b) { return sg_pc_d2(a[0], a[1], a[2], b[0], b[1], b[2]); }

// the header's summation order of the minima m[0..n): tiles of 2048, 256 strided partial sums, a halving tree, tiles in order
static double cd_mean(const float* m, long n) {
    double total = 0.0;
    for (long t0 = 0; t0 < n; t0 += 2048) {
        double s[256];
        for (int l = 0; l < 256; ++l) s[l] = 0.0;
        for (int k = 0; k < 8; ++k)
            for (int l = 0; l < 256; ++l) {
                const long p = t0 + (long)k * 256 + l;
                if (p < n) s[l] += (double)m[p];
            }
        for (int off = 128; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) s[l] += s[l + off];
        total += s[0];
    }
    return total / (double)n;
}

int sg_chamfer_matrix_cpu(const float* A, const float* B, long Sa, long Sb, long P, long Q, double* ab, double* ba, void*, size_t,
                          hipStream_t_) {
    CPU_CHECK(A && B && (ab || ba) && Sa >= 1 && Sb >= 1 && P >= 1 && Q >= 1 && Sa <= 65535 && Sb <= 65535 && P <= (1L << 26) &&
              Q <= (1L << 26));
#pragma omp parallel
    {
        std::vector<float> ma((size_t)P), mb((size_t)Q);
#pragma omp for schedule(dynamic)
        for (long e = 0; e < Sa * Sb; ++e) {
            const float* a = A + (e / Sb) * P * 3;
            const float* b = B + (e % Sb) * Q * 3;
            std::fill(mb.begin(), mb.end(), INFINITY);
            for (long p = 0; p < P; ++p) {
                float best = INFINITY;
                for (long q = 0; q < Q; ++q) {
                    const float d = cd_pair(a + p * 3, b + q * 3);
                    best = d < best ? d : best;
                    mb[q] = d < mb[q] ? d : mb[q];
                }
                ma[p] = best;
            }
            if (ab) ab[e] = cd_mean(ma.data(), P);
            if (ba) ba[e] = cd_mean(mb.data(), Q);
        }
    }
    return SG_OK;
}

static void cd_nearest(const float* A, const float* B, long S, long P, long Q, float* dist, int* idx) {
#pragma omp parallel for schedule(static)
    for (long r = 0; r < S * P; ++r) {
        const float* a = A + r * 3;
        const float* b = B + (r / P) * Q * 3;
        float best = INFINITY;
        int arg = 0;
        for (long q = 0; q < Q; ++q) {
            const float d = cd_pair(a, b + q * 3);
            if (d < best) {      // increasing index, strict: the lowest index of a tie stays
                best = d;
                arg = (int)q;
            }
        }
        dist[r] = best;
        idx[r] = arg;
    }
}

int sg_chamfer_nearest_cpu(const float* A, const float* B, long S, long P, long Q, float* dist_a, int* idx_a, float* dist_b, int* idx_b,
                           hipStream_t_) {
    CPU_CHECK(A && B && S >= 1 && S <= 65535 && P >= 1 && Q >= 1 && P <= (1L << 26) && Q <= (1L << 26));
    CPU_CHECK((dist_a != nullptr) == (idx_a != nullptr) && (dist_b != nullptr) == (idx_b != nullptr) && (dist_a || dist_b));
    if (dist_a) cd_nearest(A, B, S, P, Q, dist_a, idx_a);
    if (dist_b) cd_nearest(B, A, S, Q, P, dist_b, idx_b);
    return SG_OK;
}

int sg_occupancy_histogram_cpu(const float* clouds, long S, long P, int R, int64_t* hist, hipStream_t_) {
    CPU_CHECK(clouds && hist && S >= 1 && P >= 1 && R >= 2 && R <= 1024 && S * P <= (1L << 38));
    const float rm1 = (float)(R - 1);
    for (long i = 0; i < S * P; ++i) {
        const int ix = sg_pc_occupancy_axis(clouds[i * 3], rm1), iy = sg_pc_occupancy_axis(clouds[i * 3 + 1], rm1),
                  iz = sg_pc_occupancy_axis(clouds[i * 3 + 2], rm1);
        hist[((long)ix * R + iy) * R + iz] += 1;
    }
    return SG_OK;
}

// ---- K15: earth mover's distance (include/shapegan_hip.h): the same rounds as csrc/emd.hip, from a table of the integer costs ----
struct EmdScratch {
    std::vector<int> cost, price, owner, asg, list;
    std::vector<uint64_t> bid;
    std::vector<float> d;
};

static void emd_pair(const float* a, const float* b, int P, float u, int* match, double* emd, int* rounds, int* status, EmdScratch& w) {
    w.cost.resize((size_t)P * P);
    int kmax = 0;
    bool too_small = false;
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            const float d = sqrtf(cd_pair(a + i * 3, b + j * 3));
            const int k = sg_emd_cost(d, u);
            too_small |= sg_emd_too_small(d, u);
            w.cost[(size_t)i * P + j] = k;
            kmax = k > kmax ? k : kmax;
        }
    w.asg.resize(P);
    for (int i = 0; i < P; ++i) w.asg[i] = i;
    int total = 0, st = too_small ? 2 : 0;
    if (!too_small) {
        w.price.assign(P, 0);
        w.bid.assign(P, 0);
        w.owner.resize(P);
        for (int e = kmax >> 4 > 1 ? kmax >> 4 : 1; st == 0; e = e >> 2 > 1 ? e >> 2 : 1) {
            for (int i = 0; i < P; ++i) w.owner[i] = -1, w.asg[i] = i;
            for (int r = 0;; ++r) {
                w.list.clear();
                for (int i = 0; i < P; ++i)
                    if (w.owner[w.asg[i]] != i) w.list.push_back(i);
                if (w.list.empty()) break;
                if (r == SG_EMD_ROUND_CAP) {
                    st = 1;
                    break;
                }
                ++total;
                for (int i : w.list) {
                    const int* c = &w.cost[(size_t)i * P];
                    int w1 = INT32_MIN, w2 = INT32_MIN, j1 = 0;
                    for (int j = 0; j < P; ++j) {       // increasing j, strict: the lowest j of a tie stays
                        const int v = -c[j] - w.price[j];
                        if (v > w1) {
                            w2 = w1;
                            w1 = v;
                            j1 = j;
                        } else if (v > w2) {
                            w2 = v;
                        }
                    }
                    if (w2 == INT32_MIN) w2 = w1;       // P = 1
                    // (bid, 65535 - bidder): one maximum picks the highest bid and, among equals, the lowest bidder
                    const uint64_t word = ((uint64_t)(uint32_t)(w.price[j1] + (w1 - w2) + e) << 32) | (uint32_t)(0xFFFF - i);
                    w.bid[j1] = word > w.bid[j1] ? word : w.bid[j1];
                    w.asg[i] = j1;
                }
                for (int j = 0; j < P; ++j)
                    if (w.bid[j]) {
                        w.price[j] = (int)(w.bid[j] >> 32);
                        w.owner[j] = 0xFFFF - (int)(w.bid[j] & 0xFFFF);
                        w.bid[j] = 0;
                    }
            }
            if (e == 1) break;
        }
    }
    if (st == 0) {
        w.d.resize(P);
        for (int i = 0; i < P; ++i) w.d[i] = sqrtf(cd_pair(a + i * 3, b + w.asg[i] * 3));
        *emd = cd_mean(w.d.data(), P);
    } else {
        *emd = NAN;
    }
    if (match)
        for (int i = 0; i < P; ++i) match[i] = w.asg[i];
    if (rounds) *rounds = total;
    *status = st;
}

static bool emd_args_ok(long S, long P, double eps, const char* who) {
    const int refused = sg_emd_refused(S, P, eps);
    if (refused == 1)
        snprintf(g_err, sizeof(g_err), "%s: 1 <= P <= %d points per cloud and at most 65535 clouds per call, got P = %ld", who,
                 SG_EMD_MAX_POINTS, P);
    else if (refused)
        snprintf(g_err, sizeof(g_err), "%s: eps must be a finite number of at least 4.8e-38, got %g", who, eps);
    return !refused;
}

int sg_emd_match_cpu(const float* A, const float* B, long S, long P, double eps, int* match, double* emd, int* rounds, int* status,
                     hipStream_t_) {
    CPU_CHECK(A && B && emd && status);
    if (!emd_args_ok(S, P, eps, __func__)) return SG_ERR_ARG;
    const float u = sg_emd_unit(eps);
#pragma omp parallel
    {
        EmdScratch w;
#pragma omp for schedule(dynamic)
        for (long s = 0; s < S; ++s)
            emd_pair(A + s * P * 3, B + s * P * 3, (int)P, u, match ? match + s * P : nullptr, emd + s, rounds ? rounds + s : nullptr,
                     status + s, w);
    }
    return SG_OK;
}

int sg_emd_matrix_cpu(const float* A, const float* B, long Sa, long Sb, long P, double eps, int symmetric, double* emd, int* status,
                      void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(A && B && emd && status && workspace && Sb >= 1 && Sb <= 65535 && (!symmetric || Sa == Sb));
    if (!emd_args_ok(Sa, P, eps, __func__)) return SG_ERR_ARG;
    CPU_CHECK(workspace_bytes >= (size_t)(Sa * Sb) * sizeof(int));
    const float u = sg_emd_unit(eps);
    int* rounds = (int*)workspace;
#pragma omp parallel
    {
        EmdScratch w;
#pragma omp for schedule(dynamic)
        for (long e = 0; e < Sa * Sb; ++e) {
            const long i = e / Sb, j = e % Sb;
            if (symmetric && i >= j) {
                if (i == j) emd[e] = 0.0, status[e] = 0, rounds[e] = 0;
                continue;
            }
            emd_pair(A + i * P * 3, B + j * P * 3, (int)P, u, nullptr, emd + e, rounds + e, status + e, w);
            if (symmetric) emd[j * Sb + i] = emd[e], status[j * Sb + i] = status[e], rounds[j * Sb + i] = rounds[e];
        }
    }
    return SG_OK;
}
#pragma GCC pop_options

}  // extern "C"

// ---- K14: tiled rasteriser (include/shapegan_hip.h) --------------------------------------------------------------------------------
// The per-triangle and per-sample arithmetic is csrc/raster_core.h, the file the HIP kernels include: one statement of every fp32
// formula, like the areas above.  What is written here: the loops, the bins (filled in triangle order) and the search for the winner.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/raster_core.h"

static inline int rs_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline bool rs_view_ok(long S, long T, int W, int H) {
    return S >= 1 && S <= 65535 && T >= 0 && T <= 2147483647L && W >= 1 && H >= 1 && W <= 16384 && H <= 16384 &&
           S * (long)rs_cdiv(W, SG_RS_TILE) * rs_cdiv(H, SG_RS_TILE) <= 2147483647L;
}

extern "C" {

int sg_raster_setup_cpu(const float* positions, const int64_t* tri_offsets, long S, long T, const double* vp, int width, int height,
                        int cull_back, double near_w, int* recs, int* flags, float* clip, int* dropped, float* ground, int* tile_counts,
                        hipStream_t_) {
    CPU_CHECK(rs_view_ok(S, T, width, height) && tri_offsets && vp && dropped && tile_counts);
    CPU_CHECK(T == 0 || (positions && recs && flags));
    float M[16];
    for (int i = 0; i < 16; ++i) M[i] = (float)vp[i];
    const int ntx = rs_cdiv(width, SG_RS_TILE), nty = rs_cdiv(height, SG_RS_TILE);
    std::fill(tile_counts, tile_counts + S * (long)ntx * nty, 0);
    SgRasterRec* R = (SgRasterRec*)recs;
#pragma omp parallel for schedule(static)
    for (long t = 0; t < T; ++t) flags[t] = sg_rs_setup(positions + t * 9, M, width, height, cull_back, (float)near_w, &R[t], clip ? clip + t * 12 : nullptr);
    for (long s = 0; s < S; ++s) {
        dropped[s] = 0;
        float g = INFINITY;
        int* counts = tile_counts + s * (long)ntx * nty;
        const long t0 = std::max<long>(tri_offsets[s], 0), t1 = std::min<long>(tri_offsets[s + 1], T);
        for (long t = t0; t < t1; ++t) {
            for (int k = 0; k < 3; ++k) g = std::min(g, positions[t * 9 + k * 3 + 1]);
            if (flags[t] & SG_RS_DROPPED) dropped[s] += 1;
            if (flags[t]) continue;
            for (int ty = R[t].py0 >> SG_RS_TILE_SHIFT; ty <= R[t].py1 >> SG_RS_TILE_SHIFT; ++ty)
                for (int tx = R[t].px0 >> SG_RS_TILE_SHIFT; tx <= R[t].px1 >> SG_RS_TILE_SHIFT; ++tx) counts[ty * ntx + tx] += 1;
        }
        if (ground) ground[s] = t1 > t0 ? g : -1.0f;
    }
    return SG_OK;
}

int sg_raster_scan_cpu(const int* tile_counts, long ntiles, int64_t* tile_offsets, int* cursor, int* active, int64_t* totals,
                       hipStream_t_) {
    CPU_CHECK(tile_counts && tile_offsets && cursor && active && totals && ntiles >= 1 && ntiles <= 2147483647L);
    int64_t run = 0, nact = 0;
    for (long i = 0; i < ntiles; ++i) {
        const int c = tile_counts[i] > 0 ? tile_counts[i] : 0;
        tile_offsets[i] = run;
        cursor[i] = 0;
        if (c > 0) active[nact++] = (int)i;
        run += c;
    }
    tile_offsets[ntiles] = run;
    totals[0] = run;
    totals[1] = nact;
    return SG_OK;
}

int sg_raster_fill_cpu(const int* recs, const int* flags, const int64_t* tri_offsets, long S, long T, int width, int height,
                       const int64_t* tile_offsets, int* cursor, int* lists, long capacity, hipStream_t_) {
    CPU_CHECK(rs_view_ok(S, T, width, height) && tri_offsets && tile_offsets && cursor && capacity >= 0);
    if (T == 0 || capacity == 0) return SG_OK;
    CPU_CHECK(recs && flags && lists);
    const SgRasterRec* R = (const SgRasterRec*)recs;
    const int ntx = rs_cdiv(width, SG_RS_TILE), nty = rs_cdiv(height, SG_RS_TILE);
    for (long s = 0; s < S; ++s) {
        const long t0 = std::max<long>(tri_offsets[s], 0), t1 = std::min<long>(tri_offsets[s + 1], T);
        for (long t = t0; t < t1; ++t) {
            if (flags[t]) continue;
            const SgRasterRec& r = R[t];
            if (r.px0 < 0 || r.py0 < 0 || (r.px1 >> SG_RS_TILE_SHIFT) >= ntx || (r.py1 >> SG_RS_TILE_SHIFT) >= nty) continue;
            for (int ty = r.py0 >> SG_RS_TILE_SHIFT; ty <= r.py1 >> SG_RS_TILE_SHIFT; ++ty)
                for (int tx = r.px0 >> SG_RS_TILE_SHIFT; tx <= r.px1 >> SG_RS_TILE_SHIFT; ++tx) {
                    const long g = s * (long)ntx * nty + ty * ntx + tx;
                    const long at = tile_offsets[g] + cursor[g]++;
                    if (at >= tile_offsets[g] && at < tile_offsets[g + 1] && at < capacity) lists[at] = (int)t;
                }
        }
    }
    return SG_OK;
}

int sg_raster_visibility_cpu(const int* recs, const int64_t* tri_offsets, long S, int width, int height, const int64_t* tile_offsets,
                             const int* lists, long capacity, const int* active, long nactive, int* id, float* depth, int shadow,
                             hipStream_t_) {
    CPU_CHECK(rs_view_ok(S, 0, width, height) && tri_offsets && tile_offsets && depth && capacity >= 0 && nactive >= 0);
    const int ntx = rs_cdiv(width, SG_RS_TILE), nty = rs_cdiv(height, SG_RS_TILE);
    const long ntiles = (long)ntx * nty;
    CPU_CHECK(nactive <= S * ntiles && (nactive == 0 || (recs && lists && active)));
    const SgRasterRec* R = (const SgRasterRec*)recs;
    const long n = S * (long)height * width;
    for (long i = 0; i < n; ++i) {
        if (id) id[i] = -1;
        depth[i] = 1.0f;
    }
#pragma omp parallel for schedule(dynamic)
    for (long a = 0; a < nactive; ++a) {
        const long g = active[a];
        if (g < 0 || g >= S * ntiles) continue;
        const long s = g / ntiles;
        const int tile = (int)(g - s * ntiles), tx = tile % ntx, ty = tile / ntx;
        const long begin = std::max<long>(tile_offsets[g], 0), end = std::min<long>(tile_offsets[g + 1], capacity);
        for (int ly = 0; ly < SG_RS_TILE; ++ly)
            for (int lx = 0; lx < SG_RS_TILE; ++lx) {
                const int px = tx * SG_RS_TILE + lx, py = ty * SG_RS_TILE + ly;
                if (px >= width || py >= height) continue;
                float best = INFINITY;
                int best_id = -1;
                for (long c = begin; c < end; ++c) {
                    const long t = lists[c];
                    if (t < tri_offsets[s] || t >= tri_offsets[s + 1]) continue;
                    const SgRasterRec& r = R[t];
                    if (px < r.px0 || px > r.px1 || py < r.py0 || py > r.py1) continue;
                    int64_t e[3], a2;
                    if (!sg_rs_cover(r.x, r.y, px, py, e, &a2)) continue;
                    const float z = sg_rs_depth(e, 1.0f / (float)a2, r.z[0], r.z[1] - r.z[0], r.z[2] - r.z[0]);
                    if (z < best || (z == best && (int)t < best_id)) {
                        best = z;
                        best_id = (int)t;
                    }
                }
                const long o = (s * height + py) * width + px;
                if (id) id[o] = best_id;
                depth[o] = best_id < 0 ? 1.0f : (shadow ? fmaf(0.5f, best, 0.5f) : best);
            }
    }
    return SG_OK;
}

int sg_raster_shade_cpu(const float* positions, const float* normals, long T, const int* recs, const int* id, const float* depth,
                        const float* shadow_map, int shadow_size, const float* ground, const double* params, long S, int width,
                        int height, unsigned char* image, hipStream_t_) {
    CPU_CHECK(rs_view_ok(S, T, width, height) && id && depth && shadow_map && shadow_size >= 1 && shadow_size <= 16384 && ground &&
              params && image);
    CPU_CHECK(T == 0 || (positions && recs));
    SgRasterParams P;
    sg_rs_params_from_host(params, &P);
    const long n = S * (long)height * width;
#pragma omp parallel for schedule(static)
    for (long i = 0; i < n; ++i) {
        const long s = i / ((long)height * width);
        const int rem = (int)(i - s * height * width), py = rem / width, px = rem - py * width;
        sg_rs_shade(px, py, width, height, id[i], depth[i], T, (const SgRasterRec*)recs, positions, normals,
                    shadow_map + s * (long)shadow_size * shadow_size, shadow_size, ground[s], P, image + i * 3);
    }
    return SG_OK;
}

int sg_raster_resolve_cpu(const unsigned char* samples, long S, int width, int height, int ssaa, unsigned char* image, hipStream_t_) {
    CPU_CHECK(samples && image && S >= 1 && width >= 1 && height >= 1 && ssaa >= 1 && ssaa <= 16 && (long)width * ssaa <= 16384 &&
              (long)height * ssaa <= 16384);
    const long Wi = (long)width * ssaa, n = ssaa * ssaa;
#pragma omp parallel for schedule(static)
    for (long q = 0; q < S * (long)height * width; ++q) {
        const long s = q / ((long)height * width);
        const int rem = (int)(q - s * height * width), y = rem / width, x = rem - y * width;
        for (int c = 0; c < 3; ++c) {
            long sum = 0;
            for (int a = 0; a < ssaa; ++a)
                for (int b = 0; b < ssaa; ++b) sum += samples[((s * height * ssaa + (long)y * ssaa + a) * Wi + (long)x * ssaa + b) * 3 + c];
            image[q * 3 + c] = (unsigned char)((2 * sum + n) / (2 * n));
        }
    }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options

// ---- K16: meshes to signed distances (include/shapegan_hip.h) ----------------------------------------------------------------------
// The per-pair arithmetic is csrc/meshsdf_core.h, the file csrc/meshsdf.hip includes.  Here: the records, the walk over a shape's
// triangles in increasing index with a strict comparison, and the loop over the scans.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/meshsdf_core.h"

extern "C" {

int sg_meshsdf_distance_cpu(const float* positions, const int64_t* tri_offsets, long S, long T, const float* points, long Q, float* dist2,
                            int* tri, float* closest, void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(sg_msdf_sizes_ok(S, T, Q));
    CPU_CHECK(tri_offsets && points && dist2 && workspace && (T == 0 || positions));
    CPU_CHECK(workspace_bytes >= (size_t)T * sizeof(SgMsdfRec));      // the twin keeps its records where the library does
    SgMsdfRec* recs = (SgMsdfRec*)workspace;
#pragma omp parallel for schedule(static)
    for (long t = 0; t < T; ++t) sg_msdf_record(positions + t * 9, &recs[t]);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < S * Q; ++i) {
        const long s = i / Q;
        const long t0 = std::max<long>(tri_offsets[s], 0), t1 = std::min<long>(tri_offsets[s + 1], T);
        const float px = points[i * 3], py = points[i * 3 + 1], pz = points[i * 3 + 2];
        float best = INFINITY, c[3] = {0.f, 0.f, 0.f};
        long arg = -1;
        for (long t = t0; t < t1; ++t) {
            const float d2 = sg_msdf_d2(px, py, pz, recs[t], nullptr);
            if (d2 < best) {
                best = d2;
                arg = t - t0;
            }
        }
        if (arg >= 0 && closest) sg_msdf_d2(px, py, pz, recs[t0 + arg], c);
        dist2[i] = best;
        if (tri) tri[i] = (int)arg;
        if (closest) closest[i * 3] = c[0], closest[i * 3 + 1] = c[1], closest[i * 3 + 2] = c[2];
    }
    return SG_OK;
}

int sg_meshsdf_sign_cpu(const float* points, long S, long Q, const float* depth, const double* vps, int K, int N, float bias,
                        const float* dist2, float* sdf, unsigned char* outside, hipStream_t_) {
    CPU_CHECK(sg_msdf_sizes_ok(S, 0, Q) && sg_msdf_scans_ok(vps, K, N, bias));
    CPU_CHECK(points && depth && (sdf != nullptr) == (dist2 != nullptr) && (sdf || outside));
    std::vector<float> M((size_t)K * 12);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < 12; ++i) M[(size_t)k * 12 + i] = (float)vps[k * 16 + i];
#pragma omp parallel for schedule(static)
    for (long i = 0; i < S * Q; ++i) {
        const long s = i / Q;
        bool seen = false;
        for (int k = 0; k < K && !seen; ++k)
            seen = sg_msdf_visible(&M[(size_t)k * 12], points[i * 3], points[i * 3 + 1], points[i * 3 + 2], depth + ((long)k * S + s) * N * N, N, bias);
        if (outside) outside[i] = seen ? 1 : 0;
        if (sdf) {
            const float d = sqrtf(dist2[i]);
            sdf[i] = seen ? d : -d;
        }
    }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options

// ---- K17: exact t-SNE ------------------------------------------------------------------------------------------------------------
// The per-element arithmetic is csrc/tsne_core.h, the file csrc/tsne.hip includes.  Here: plain loops over rows (OpenMP), a row's sums
// as float partial sums over SG_TSNE_FLUSH columns flushed into float64, rows added in increasing index.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/tsne_core.h"

extern "C" {

int sg_tsne_affinities_cpu(const float* X, long N, long D, double perplexity, double tol, int max_steps, float* P, float* beta,
                           double* plogp, void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(sg_tsne_sizes_ok(N, D, perplexity));
    CPU_CHECK(X && P && beta && plogp && workspace && tol >= 0.0 && max_steps >= 1);
    CPU_CHECK(workspace_bytes >= (size_t)N * sizeof(double));
    double* rows = (double*)workspace;
    const double log_perp = log(perplexity);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < N; ++i)
        for (long j = 0; j < N; ++j) {
            float acc = 0.f;
            for (long k = 0; k < D; ++k) acc = sg_tsne_d2_step(acc, X[i * D + k], X[j * D + k]);
            P[i * N + j] = acc;
        }
#pragma omp parallel for schedule(static)
    for (long i = 0; i < N; ++i) {
        float* row = P + i * N;
        float m = INFINITY;
        for (long j = 0; j < N; ++j)
            if (j != i) m = fminf(m, row[j]);
        SgTsneSearch st;
        sg_tsne_search_init(&st);
        double sum_p = 1.0;
        for (int step = 0;; ++step) {
            double sp = 0.0, sdp = 0.0;
            for (long j = 0; j < N; ++j)
                if (j != i) {
                    const float d = row[j] - m;
                    const float p = sg_tsne_cond(st.beta, d);
                    sp += (double)p;
                    sdp += (double)d * (double)p;
                }
            sum_p = sp;
            if (step + 1 >= max_steps) break;
            if (sg_tsne_search_next(&st, sg_tsne_entropy(st.beta, sp, sdp) - log_perp, tol)) break;
        }
        for (long j = 0; j < N; ++j) row[j] = j == i ? 0.f : (float)((double)sg_tsne_cond(st.beta, row[j] - m) / sum_p);
        beta[i] = st.beta;
    }
    const float two_n = (float)(2 * N);
#pragma omp parallel for schedule(dynamic, 16)
    for (long i = 0; i < N; ++i)
        for (long j = i; j < N; ++j) {      // the pair (i, j), i <= j, is written by this iteration alone
            const float v = sg_tsne_joint(P[i * N + j], P[j * N + i], two_n);
            P[i * N + j] = v;
            P[j * N + i] = v;
        }
#pragma omp parallel for schedule(static)
    for (long i = 0; i < N; ++i) {
        double s = 0.0;
        for (long j = 0; j < N; ++j) {
            const float p = P[i * N + j];
            if (p > 0.f) s += (double)p * log((double)p);
        }
        rows[i] = s;
    }
    double total = 0.0;
    for (long i = 0; i < N; ++i) total += rows[i];
    *plogp = total;
    return SG_OK;
}

static void tsne_rows_cpu(const float* Y, const float* P, long N, bool want_k, double* stats) {
#pragma omp parallel for schedule(static)
    for (long i = 0; i < N; ++i) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        const float yix = Y[2 * i], yiy = Y[2 * i + 1];
        for (long j0 = 0; j0 < N; j0 += SG_TSNE_FLUSH) {
            SgTsneAcc a;
            sg_tsne_acc_zero(&a);
            const long j1 = std::min<long>(N, j0 + SG_TSNE_FLUSH);
            if (want_k)
                for (long j = j0; j < j1; ++j) sg_tsne_pair<true>(&a, yix, yiy, Y[2 * j], Y[2 * j + 1], P[i * N + j], j != i);
            else
                for (long j = j0; j < j1; ++j) sg_tsne_pair<false>(&a, yix, yiy, Y[2 * j], Y[2 * j + 1], P[i * N + j], j != i);
            acc[0] += (double)a.s, acc[1] += (double)a.ax, acc[2] += (double)a.ay;
            acc[3] += (double)a.rx, acc[4] += (double)a.ry, acc[5] += (double)a.k;
        }
        for (int e = 0; e < 6; ++e) stats[i * 6 + e] = acc[e];
    }
}

static int tsne_gradient_cpu(float* Y, const float* P, long N, float exaggeration, const double* plogp, float* velocity, float* gains,
                             float momentum, float lr, float min_gain, bool update, float* grad, double* kl, void* workspace) {
    double* stats = (double*)workspace;
    tsne_rows_cpu(Y, P, N, kl != nullptr, stats);
    double Z = 0.0, K = 0.0;
    for (long i = 0; i < N; ++i) Z += stats[i * 6], K += stats[i * 6 + 5];
    stats[6 * N] = Z;
    if (kl) *kl = *plogp + K + log(Z);
    for (long i = 0; i < N; ++i)
        for (int c = 0; c < 2; ++c) {
            const float g = sg_tsne_grad(stats[i * 6 + 1 + c], stats[i * 6 + 3 + c], Z, exaggeration);
            grad[2 * i + c] = g;
            if (update) sg_tsne_update_one(Y + 2 * i + c, velocity + 2 * i + c, gains + 2 * i + c, g, momentum, lr, min_gain);
        }
    return SG_OK;
}

int sg_tsne_gradient_cpu(const float* Y, const float* P, long N, float exaggeration, const double* plogp, float* grad, double* kl,
                         void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(N >= 4 && N <= SG_TSNE_MAX_POINTS && Y && P && grad && workspace);
    CPU_CHECK(!kl || plogp);
    CPU_CHECK(workspace_bytes >= ((size_t)6 * N + 2) * sizeof(double));
    return tsne_gradient_cpu((float*)Y, P, N, exaggeration, plogp, nullptr, nullptr, 0.f, 0.f, 0.f, false, grad, kl, workspace);
}

int sg_tsne_update_cpu(float* Y, float* velocity, float* gains, const float* grad, long N, float momentum, float lr, float min_gain,
                       hipStream_t_) {
    CPU_CHECK(N >= 1 && N <= SG_TSNE_MAX_POINTS && Y && velocity && gains && grad);
    for (long e = 0; e < 2 * N; ++e) sg_tsne_update_one(Y + e, velocity + e, gains + e, grad[e], momentum, lr, min_gain);
    return SG_OK;
}

int sg_tsne_step_cpu(float* Y, const float* P, long N, float exaggeration, const double* plogp, float* velocity, float* gains,
                     float momentum, float lr, float min_gain, float* grad, double* kl, void* workspace, size_t workspace_bytes,
                     hipStream_t_) {
    CPU_CHECK(N >= 4 && N <= SG_TSNE_MAX_POINTS && Y && P && velocity && gains && grad && workspace);
    CPU_CHECK(!kl || plogp);
    CPU_CHECK(workspace_bytes >= ((size_t)6 * N + 2) * sizeof(double));
    return tsne_gradient_cpu(Y, P, N, exaggeration, plogp, velocity, gains, momentum, lr, min_gain, true, grad, kl, workspace);
}

}  // extern "C"
#pragma GCC pop_options

// ---- K18: narrow-band voxel grids (csrc/brickgrid.hip) --------------------------------------------------------------------------------
// The integer and side-of-level arithmetic is csrc/brickgrid_core.h, the file the HIP kernels include.  Here: plain walks over the
// bricks in ascending order (which is the order the HIP scan produces).
#include "../csrc/brickgrid_core.h"

extern "C" {

int sg_brick_points_cpu(const int* bricks, long M, int corners, long S, int R, int B, const float* axis_x, const float* axis_y,
                        const float* axis_z, float* points, int* shape_index, hipStream_t_) {
    SgBrickGeom g;
    CPU_CHECK(sg_brick_geom(g, S, R, B));
    CPU_CHECK(axis_x && axis_y && axis_z && points && shape_index && M > 0 && M <= g.S * g.nb && (corners == 0 || corners == 1));
    CPU_CHECK(bricks || M == g.S * g.nb);
    const long ppb = corners ? 8 : (long)B * B * B;
#pragma omp parallel for schedule(static)
    for (long j = 0; j < M; ++j) {
        const long brick = bricks ? (long)bricks[j] : j;
        if (brick < 0 || brick >= g.S * g.nb) continue;
        long s;
        int bx, by, bz;
        sg_brick_decode(g, brick, s, bx, by, bz);
        for (int l = 0; l < ppb; ++l) {
            int lx, ly, lz;
            if (corners) {
                sg_brick_corner_local(g, l, lx, ly, lz);
            } else {
                lx = l / (B * B);
                ly = (l / B) % B;
                lz = l % B;
            }
            const long i = j * ppb + l;
            points[i * 3] = axis_x[bx * B + lx];
            points[i * 3 + 1] = axis_y[by * B + ly];
            points[i * 3 + 2] = axis_z[bz * B + lz];
            shape_index[i] = (int)s;
        }
    }
    return SG_OK;
}

int sg_brick_seed_cpu(const float* corner_values, const unsigned char* mask, long S, int R, int B, float level, float band, int pad,
                      int* state, float* fill, int* flag, float* grid, hipStream_t_) {
    SgBrickGeom g;
    CPU_CHECK(sg_brick_geom(g, S, R, B));
    CPU_CHECK(corner_values && state && fill && flag && grid && band >= 0.f && (pad == 0 || pad == 1) && S <= 65535);
    const long cells = (long)R * R * R;
#pragma omp parallel for schedule(static)
    for (long brick = 0; brick < g.S * g.nb; ++brick) {
        long s;
        int bx, by, bz;
        sg_brick_decode(g, brick, s, bx, by, bz);
        float f;
        flag[brick] = sg_brick_seed_test(g, corner_values, mask, s, bx, by, bz, level, band, pad, &f) ? 1 : 0;
        fill[brick] = f;
        state[brick] = 0;
    }
#pragma omp parallel for schedule(static)
    for (long brick = 0; brick < g.S * g.nb; ++brick) {
        long s;
        int bx, by, bz;
        sg_brick_decode(g, brick, s, bx, by, bz);
        for (int l = 0; l < B * B * B; ++l) {
            const long p = sg_brick_lattice(g, bx, by, bz, l / (B * B), (l / B) % B, l % B);
            grid[s * cells + p] = (mask && !mask[p]) ? 1.f : fill[brick];
        }
    }
    return SG_OK;
}

int sg_brick_compact_cpu(int* state, int* flag, long S, int R, int B, int* list, int* count, void* workspace, size_t, hipStream_t_) {
    SgBrickGeom g;
    CPU_CHECK(sg_brick_geom(g, S, R, B));
    CPU_CHECK(state && flag && list && count && workspace);
    int n = 0;
    for (long i = 0; i < g.S * g.nb; ++i) {
        if (flag[i]) {
            list[n++] = (int)i;
            state[i] = 2;
            flag[i] = 0;
        } else if (state[i] == 2) {
            state[i] = 1;
        }
    }
    *count = n;
    return SG_OK;
}

int sg_brick_scatter_cpu(const float* values, const int* bricks, long M, const unsigned char* mask, long S, int R, int B, float* grid,
                         hipStream_t_) {
    SgBrickGeom g;
    CPU_CHECK(sg_brick_geom(g, S, R, B));
    CPU_CHECK(values && bricks && grid && M > 0 && M <= g.S * g.nb);
    const long cells = (long)R * R * R, ppb = (long)B * B * B;
#pragma omp parallel for schedule(static)
    for (long j = 0; j < M; ++j) {
        const long brick = bricks[j];
        if (brick < 0 || brick >= g.S * g.nb) continue;
        long s;
        int bx, by, bz;
        sg_brick_decode(g, brick, s, bx, by, bz);
        for (int l = 0; l < ppb; ++l) {
            const long p = sg_brick_lattice(g, bx, by, bz, l / (B * B), (l / B) % B, l % B);
            grid[s * cells + p] = (mask && !mask[p]) ? 1.f : values[j * ppb + l];
        }
    }
    return SG_OK;
}

int sg_brick_grow_cpu(const int* bricks, long M, const float* grid, const int* state, const float* fill, long S, int R, int B, float level,
                      int* flag, hipStream_t_) {
    SgBrickGeom g;
    CPU_CHECK(sg_brick_geom(g, S, R, B));
    CPU_CHECK(bricks && grid && state && fill && flag && M > 0 && M <= g.S * g.nb);
    const long cells = (long)R * R * R;
    for (long j = 0; j < M; ++j) {
        const long brick = bricks[j];
        if (brick < 0 || brick >= g.S * g.nb) continue;
        long s;
        int bx, by, bz;
        sg_brick_decode(g, brick, s, bx, by, bz);
        unsigned in_mask = 0, out_mask = 0;
        for (int l = 0; l < B * B * B; ++l) {
            const int lx = l / (B * B), ly = (l / B) % B, lz = l % B;
            const unsigned m = sg_brick_region_mask(B, lx, ly, lz);
            if (sg_brick_inside(grid[s * cells + sg_brick_lattice(g, bx, by, bz, lx, ly, lz)], level))
                in_mask |= m;
            else
                out_mask |= m;
        }
        for (int d = 0; d < 27; ++d) sg_brick_grow_apply(g, state, fill, flag, brick, d, in_mask, out_mask, level);
    }
    return SG_OK;
}

}  // extern "C"

// ---- K7d: points onto a level set of a frozen SDFNet (header: sg_sdfnet_project; csrc/sdfnet_project.hip) ----------------------------
// Per point of every tile the caller's table names: `iterations + 1` rounds of the forward of sg_sdfnet_fwd_cpu (the same `dense`
// calls in the same order, so iterations == 0 gives its bits), the chain of sg_sdfnet_latent_grad_cpu from dz8 = 1 - out^2, the two
// products with the point columns of W5 / W1, and between rounds the step of csrc/project_core.h, the file the HIP kernel includes.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/project_core.h"

extern "C" {

int sg_sdfnet_project_cpu(const float* points, const int64_t* seg_off, long nshapes, const float* zb1, const float* zb5,
                          const float* packed, float level, int iterations, int rule, float max_step, const int* tiles, long ntiles,
                          float* out_points, float* value, float* grad, void*) {
    CPU_CHECK(points && seg_off && zb1 && zb5 && packed && tiles && value && grad);
    CPU_CHECK(nshapes >= 1 && ntiles >= 1 && ntiles < (1L << 31));
    CPU_CHECK(iterations >= 0 && iterations <= 64 && (rule == SG_PROJECT_RULE_NEWTON || rule == SG_PROJECT_RULE_UNIT));
    CPU_CHECK(max_step >= 0.f && (out_points || iterations == 0));
    const CpuSdf v = sdf_view(packed, 3);
#pragma omp parallel for schedule(dynamic)
    for (long t = 0; t < ntiles; ++t) {
        const long s = tiles[2 * t], i0 = tiles[2 * t + 1];
        if (s < 0 || s >= nshapes || i0 < 0) continue;
        const long beg = seg_off[s], n = seg_off[s + 1] - beg;
        long cnt = n - i0;
        if (cnt > SG_SDFNET_PROJECT_TILE) cnt = SG_SDFNET_PROJECT_TILE;
        if (cnt <= 0) continue;
        float xs[SG_SDFNET_PROJECT_TILE][3];      // (all of the tile's points are read before any is written: out_points may alias)
        for (long i = 0; i < cnt; ++i)
            for (int c = 0; c < 3; ++c) xs[i][c] = points[(beg + i0 + i) * 3 + c];
        for (long i = 0; i < cnt; ++i) {
            const long pi = beg + i0 + i;
            float* x = xs[i];
            float o = 0.f, gp[3] = {0.f, 0.f, 0.f};
            for (int round = 0; round <= iterations; ++round) {
                float h[7][256], g[256];
                o = tanhf(sdf_shape_point_fwd(v, x, zb1 + s * 256, zb5 + s * 256, h));
                sdf_shape_point_grad(v, h, 1.f - o * o, g, gp, [](const float*) {});
                if (round < iterations) sg_project_step(x, o, gp, level, rule, max_step);
            }
            if (out_points)
                for (int c = 0; c < 3; ++c) out_points[pi * 3 + c] = x[c];
            value[pi] = o;
            for (int c = 0; c < 3; ++c) grad[pi * 3 + c] = gp[c];
        }
    }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options

// ---- K19: signed distances from oriented point clouds (header: sg_cloud_*; csrc/cloud.hip) -------------------------------------------
// By brute force: every query against every point of its shape's cloud, the K best kept in a small array in the order (d2, index) of
// csrc/cloud_core.h; the normal of a neighbourhood and the vote of a normal are that file's, which the HIP kernels include.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/cloud_core.h"

// false when an offset table is not S runs of at most 2^26 points from 0 to total
static bool cloud_runs_ok(const int64_t* off, long S, long total) {
    if (off[0] != 0 || off[S] != total) return false;
    for (long s = 0; s < S; ++s)
        if (off[s + 1] < off[s] || off[s + 1] - off[s] > SG_CLOUD_MAX_POINTS) return false;
    return true;
}

// the first K of the cloud's points in the order (d2, index) as seen from q, `self` left out; the unused slots hold (-1, +inf)
static void cloud_list(const float* cloud, long P, const float* q, long self, int K, int* li, float* ld) {
    for (int j = 0; j < K; ++j) li[j] = -1, ld[j] = INFINITY;
    for (long p = 0; p < P; ++p) {
        if (p == self) continue;
        const float d = sg_pc_d2(q[0], q[1], q[2], cloud[p * 3], cloud[p * 3 + 1], cloud[p * 3 + 2]);
        if (!(d < INFINITY)) continue;      // NaN and +inf are never neighbours
        if (li[K - 1] >= 0 && !sg_cloud_before(d, (int)p, ld[K - 1], li[K - 1])) continue;
        int j = K - 1;
        for (; j > 0 && (li[j - 1] < 0 || sg_cloud_before(d, (int)p, ld[j - 1], li[j - 1])); --j) li[j] = li[j - 1], ld[j] = ld[j - 1];
        li[j] = (int)p, ld[j] = d;
    }
}

extern "C" {

int sg_cloud_knn_cpu(const float* points, const int64_t* cloud_offsets, const float* queries, const int64_t* query_offsets, long S, long N,
                     long M, int K, int exclude_self, int* idx, float* d2, hipStream_t_) {
    CPU_CHECK(S >= 1 && S <= 65535 && N >= 0 && M >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets && query_offsets);
    CPU_CHECK((points || N == 0) && (queries || M == 0) && ((idx && d2) || M == 0));
    CPU_CHECK(cloud_runs_ok(cloud_offsets, S, N) && cloud_runs_ok(query_offsets, S, M));
    CPU_CHECK(!exclude_self || std::equal(cloud_offsets, cloud_offsets + S + 1, query_offsets));
    for (long s = 0; s < S; ++s) {
        const long c0 = cloud_offsets[s], P = cloud_offsets[s + 1] - c0, q0 = query_offsets[s], Q = query_offsets[s + 1] - q0;
#pragma omp parallel for schedule(static)
        for (long i = 0; i < Q; ++i)
            cloud_list(points + c0 * 3, P, queries + (q0 + i) * 3, exclude_self ? i : -1, K, idx + (q0 + i) * K, d2 + (q0 + i) * K);
    }
    return SG_OK;
}

int sg_cloud_normals_cpu(const float* points, const int64_t* cloud_offsets, long S, long N, const int* idx, int K, const float* view,
                         int view_per_point, float* normals, float* variation, hipStream_t_) {
    CPU_CHECK(S >= 1 && S <= 65535 && N >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets);
    CPU_CHECK((points && idx && normals && variation) || N == 0);
    CPU_CHECK(cloud_runs_ok(cloud_offsets, S, N));
    for (long s = 0; s < S; ++s) {
        const long c0 = cloud_offsets[s], P = cloud_offsets[s + 1] - c0;
#pragma omp parallel for schedule(static)
        for (long i = 0; i < P; ++i)
            sg_cloud_normal(points + c0 * 3, P, i, idx + (c0 + i) * K, K, view ? view + (view_per_point ? c0 + i : s) * 4 : nullptr,
                            normals + (c0 + i) * 3, variation + c0 + i);
    }
    return SG_OK;
}

int sg_cloud_sdf_cpu(const float* points, const float* normals, const int64_t* cloud_offsets, const float* queries,
                     const int64_t* query_offsets, long S, long N, long M, int K, float* sdf, int* nearest, hipStream_t_) {
    CPU_CHECK(S >= 1 && S <= 65535 && N >= 0 && M >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets && query_offsets);
    CPU_CHECK(((points && normals) || N == 0) && ((queries && sdf) || M == 0));
    CPU_CHECK(cloud_runs_ok(cloud_offsets, S, N) && cloud_runs_ok(query_offsets, S, M));
    for (long s = 0; s < S; ++s) {
        const long c0 = cloud_offsets[s], P = cloud_offsets[s + 1] - c0, q0 = query_offsets[s], Q = query_offsets[s + 1] - q0;
        const float* cloud = points + c0 * 3;
        const float* cn = normals + c0 * 3;
#pragma omp parallel for schedule(static)
        for (long i = 0; i < Q; ++i) {
            const float* q = queries + (q0 + i) * 3;
            int li[SG_CLOUD_MAX_K];
            float ld[SG_CLOUD_MAX_K];
            cloud_list(cloud, P, q, -1, K, li, ld);
            int valid = 0, negative = 0;
            for (int j = 0; j < K; ++j)
                if (li[j] >= 0) {
                    const long g = (long)li[j] * 3;
                    ++valid;
                    negative += sg_cloud_vote(q[0], q[1], q[2], cloud[g], cloud[g + 1], cloud[g + 2], cn[g], cn[g + 1], cn[g + 2]) < 0.f ? 1 : 0;
                }
            sdf[q0 + i] = sg_cloud_signed(ld[0], valid, negative);
            if (nearest) nearest[q0 + i] = li[0];
        }
    }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options

// ---- K20: cubic B-spline prefilter, zoom and sampling of voxel grids (header: sg_spline_*; csrc/spline.hip) ---------------------------
// Every line filtered in place in the output, every output from its 64 taps: the formulas are csrc/spline_core.h's, which the HIP
// kernels include; the forms of the HIP library are a matter of where its lanes keep their values and do not exist here.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/spline_core.h"

static bool spline_axes_ok(long D, long H, long W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= SG_SPLINE_MAX_AXIS && H <= SG_SPLINE_MAX_AXIS && W <= SG_SPLINE_MAX_AXIS;
}
static const long kSplineMaxElements = 1L << 36;

extern "C" {

int sg_spline_prefilter_form_cpu(long D, long H, long W) {
    CPU_CHECK(spline_axes_ok(D, H, W));
    return sg_spline_prefilter_form_of(D, H, W);
}

int sg_spline_zoom_form_cpu(long D, long H, long W, long D2, long H2, long W2) {
    CPU_CHECK(spline_axes_ok(D, H, W) && spline_axes_ok(D2, H2, W2));
    return sg_spline_zoom_form_of(D, H, W, D2, H2, W2);
}

int sg_spline_prefilter_cpu(const float* grids, long S, long D, long H, long W, float* coefficients, hipStream_t_) {
    CPU_CHECK(S >= 0 && spline_axes_ok(D, H, W) && S <= kSplineMaxElements / (D * H * W));
    CPU_CHECK((grids && coefficients && grids != coefficients) || S == 0);
    const long n = D * H * W;
#pragma omp parallel for schedule(static)
    for (long s = 0; s < S; ++s) {
        float* c = coefficients + s * n;
        memcpy(c, grids + s * n, (size_t)n * sizeof(float));
        for (long r = 0; r < D * H; ++r) sg_spline_line(c + r * W, 1, (int)W);
        for (long d = 0; d < D; ++d)
            for (long w = 0; w < W; ++w) sg_spline_line(c + d * H * W + w, W, (int)H);
        for (long r = 0; r < H * W; ++r) sg_spline_line(c + r, H * W, (int)D);
    }
    return SG_OK;
}

int sg_spline_zoom_cpu(const float* coefficients, long S, long D, long H, long W, long D2, long H2, long W2, int order, float* out,
                       hipStream_t_) {
    CPU_CHECK(S >= 0 && spline_axes_ok(D, H, W) && spline_axes_ok(D2, H2, W2) && (order == 1 || order == 3));
    CPU_CHECK(S <= kSplineMaxElements / (D * H * W) && S <= kSplineMaxElements / (D2 * H2 * W2));
    CPU_CHECK((coefficients && out && coefficients != out) || S == 0);
#pragma omp parallel for collapse(2) schedule(static)
    for (long s = 0; s < S; ++s)
        for (long od = 0; od < D2; ++od) {
            int fd, fh, fw;
            float td, th, tw;
            sg_spline_coord((int)od, (int)D, (int)D2, &fd, &td);
            for (long oh = 0; oh < H2; ++oh) {
                sg_spline_coord((int)oh, (int)H, (int)H2, &fh, &th);
                for (long ow = 0; ow < W2; ++ow) {
                    sg_spline_coord((int)ow, (int)W, (int)W2, &fw, &tw);
                    out[((s * D2 + od) * H2 + oh) * W2 + ow] =
                        sg_spline_point(coefficients + s * D * H * W, (int)D, (int)H, (int)W, fd, td, fh, th, fw, tw, order, nullptr);
                }
            }
        }
    return SG_OK;
}

int sg_spline_sample_cpu(const float* coefficients, long S, long D, long H, long W, const float* points, long P, float outside,
                         float* values, float* gradient, hipStream_t_) {
    CPU_CHECK(S >= 0 && P >= 0 && spline_axes_ok(D, H, W) && S <= kSplineMaxElements / (D * H * W));
    CPU_CHECK(S == 0 || P == 0 || S <= kSplineMaxElements / (3 * P));
    CPU_CHECK((coefficients && points && values) || S == 0 || P == 0);
#pragma omp parallel for schedule(static)
    for (long i = 0; i < S * P; ++i) {
        int fd, fh, fw;
        float td, th, tw, g[3] = {0.f, 0.f, 0.f}, v = outside;
        const bool in_d = sg_spline_locate(points[i * 3], (int)D, &fd, &td), in_h = sg_spline_locate(points[i * 3 + 1], (int)H, &fh, &th),
                   in_w = sg_spline_locate(points[i * 3 + 2], (int)W, &fw, &tw);
        if (in_d && in_h && in_w)
            v = sg_spline_point(coefficients + (i / P) * D * H * W, (int)D, (int)H, (int)W, fd, td, fh, th, fw, tw, 3, gradient ? g : nullptr);
        values[i] = v;
        if (gradient) gradient[i * 3] = g[0], gradient[i * 3 + 1] = g[1], gradient[i * 3 + 2] = g[2];
    }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options

// ---- K21: distance transforms of voxel grids (header: sg_edt_*; csrc/edt.hip) ----------------------------------------------------------
// One grid at a time, every pass from one array to another, every output from csrc/edt_core.h's exact line minimum, which the HIP
// kernels include: the passes, their order and the tie rules are the header's.  The scratch is the twin's own; the caller's workspace
// is only measured, so that a short one fails here as it does on the GPU.
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#include "../csrc/edt_core.h"

static bool edt_axes_ok(long D, long H, long W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= SG_EDT_MAX_AXIS && H <= SG_EDT_MAX_AXIS && W <= SG_EDT_MAX_AXIS;
}
static bool edt_spacing_ok(float a, float b, float c) { return a > 0.f && b > 0.f && c > 0.f && a < INFINITY && b < INFINITY && c < INFINITY; }
static const long kEdtMaxElements = 1L << 36;

static size_t edt_workspace_bytes(int sites, long S, long D, long H, long W, int nearest) {
    const size_t cells = (size_t)S * D * H * W * sizeof(float);
    if (sg_edt_form_of(D, H, W) == 0) return sites == 1 && nearest ? 2 * cells : 0;
    return cells * (2 + (nearest ? (sites == 1 ? 3 : 2) : 0));
}

// one axis pass of one grid: in -> out; merge keeps what out holds unless the new value is smaller
static void edt_axis_pass(const float* in, const int* id_in, int axis, int D, int H, int W, float spacing, bool merge, float* out, int* id_out) {
    int outer, n, inner;
    sg_edt_view(axis, D, H, W, &outer, &n, &inner);
    for (int o = 0; o < outer; ++o)
        for (int p = 0; p < n; ++p)
            for (int i = 0; i < inner; ++i) {
                const long base = (long)o * n * inner + i, at = base + (long)p * inner;
                int q;
                const float r = sg_edt_axis(in + base, inner, n, p, spacing, &q);
                if (merge && !(r < out[at])) continue;
                out[at] = r;
                if (id_out) id_out[at] = id_in[base + (long)q * inner];
            }
}

extern "C" {

int sg_edt_form_cpu(long D, long H, long W) {
    CPU_CHECK(edt_axes_ok(D, H, W));
    return sg_edt_form_of(D, H, W);
}

int sg_edt_voxels_cpu(const float* grids, long S, long D, long H, long W, float level, int inside, float spacing_d, float spacing_h,
                      float spacing_w, float* squared, int* nearest, void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(S >= 0 && edt_axes_ok(D, H, W) && S <= kEdtMaxElements / (D * H * W));
    CPU_CHECK(edt_spacing_ok(spacing_d, spacing_h, spacing_w) && level == level);
    CPU_CHECK((grids && squared && grids != squared) || S == 0);
    if (S == 0) return SG_OK;
    const size_t need = edt_workspace_bytes(0, S, D, H, W, nearest != nullptr);
    if (need && (!workspace || workspace_bytes < need)) {
        snprintf(g_err, sizeof(g_err), "%s: workspace of %zu B, %zu B needed", __func__, workspace_bytes, need);
        return SG_ERR_WORKSPACE;
    }
    const long n = D * H * W;
#pragma omp parallel for schedule(static)
    for (long s = 0; s < S; ++s) {
        const float* g = grids + s * n;
        std::vector<float> A(n), B(n);
        std::vector<int> IA(nearest ? n : 0), IB(nearest ? n : 0);
        int* ia = nearest ? IA.data() : nullptr;
        int* ib = nearest ? IB.data() : nullptr;
        for (long i = 0; i < n; ++i) {
            const bool site = sg_edt_is_site(g[i], level, inside);
            A[i] = site ? 0.f : INFINITY;
            if (ia) ia[i] = site ? (int)i : -1;
        }
        edt_axis_pass(A.data(), ia, 2, (int)D, (int)H, (int)W, spacing_w, false, B.data(), ib);
        edt_axis_pass(B.data(), ib, 1, (int)D, (int)H, (int)W, spacing_h, false, A.data(), ia);
        edt_axis_pass(A.data(), ia, 0, (int)D, (int)H, (int)W, spacing_d, false, squared + s * n, nearest ? nearest + s * n : nullptr);
    }
    return SG_OK;
}

int sg_edt_crossings_cpu(const float* grids, long S, long D, long H, long W, float level, float spacing_d, float spacing_h, float spacing_w,
                         float* squared, float* closest, void* workspace, size_t workspace_bytes, hipStream_t_) {
    CPU_CHECK(S >= 0 && edt_axes_ok(D, H, W) && S <= kEdtMaxElements / (D * H * W));
    CPU_CHECK(edt_spacing_ok(spacing_d, spacing_h, spacing_w) && level == level);
    CPU_CHECK((grids && squared && grids != squared && grids != closest && squared != closest) || S == 0);
    if (S == 0) return SG_OK;
    const size_t need = edt_workspace_bytes(1, S, D, H, W, closest != nullptr);
    if (need && (!workspace || workspace_bytes < need)) {
        snprintf(g_err, sizeof(g_err), "%s: workspace of %zu B, %zu B needed", __func__, workspace_bytes, need);
        return SG_ERR_WORKSPACE;
    }
    const long n = D * H * W;
    const float sp[3] = {spacing_d, spacing_h, spacing_w};
#pragma omp parallel for schedule(static)
    for (long s = 0; s < S; ++s) {
        const float* g = grids + s * n;
        std::vector<float> A(n), B(n);
        std::vector<int> IA(closest ? n : 0), IB(closest ? n : 0), IC(closest ? n : 0);
        int* ia = closest ? IA.data() : nullptr;
        int* ib = closest ? IB.data() : nullptr;
        int* ic = closest ? IC.data() : nullptr;
        for (int axis = 0; axis < 3; ++axis) {
            int outer, len, inner;
            sg_edt_view(axis, (int)D, (int)H, (int)W, &outer, &len, &inner);
            for (long i = 0; i < n; ++i) {
                const long base = i / ((long)len * inner) * ((long)len * inner) + i % inner;
                int q;
                A[i] = sg_edt_cross(g + base, inner, len, (int)(i / inner % len), level, sp[axis], &q);
                if (ia) ia[i] = q < 0 ? -1 : sg_edt_code((int)(base + (long)q * inner), axis);
            }
            const int b = sg_edt_other_axis(axis, 0), c = sg_edt_other_axis(axis, 1);
            edt_axis_pass(A.data(), ia, b, (int)D, (int)H, (int)W, sp[b], false, B.data(), ib);
            edt_axis_pass(B.data(), ib, c, (int)D, (int)H, (int)W, sp[c], axis > 0, squared + s * n, ic);
        }
        if (closest)
            for (long i = 0; i < n; ++i) sg_edt_decode(g, (int)H, (int)W, ic[i], level, sp, closest + (s * n + i) * 3);
    }
    return SG_OK;
}

int sg_edt_finish_cpu(const float* grids, const float* squared, long S, long D, long H, long W, float level, float value_scale, int keep_band,
                      float* out, hipStream_t_) {
    CPU_CHECK(S >= 0 && edt_axes_ok(D, H, W) && S <= kEdtMaxElements / (D * H * W));
    CPU_CHECK((squared && out && (grids ? grids != out && grids != squared : keep_band == 0)) || S == 0);
    const long n = D * H * W;
    if (!grids) {      // the plain root: no sign, no band
#pragma omp parallel for schedule(static)
        for (long i = 0; i < S * n; ++i) out[i] = sg_edt_root(squared[i]);
        return SG_OK;
    }
#pragma omp parallel for collapse(2) schedule(static)
    for (long s = 0; s < S; ++s)
        for (long d = 0; d < D; ++d)
            for (long h = 0; h < H; ++h)
                for (long w = 0; w < W; ++w) {
                    const long i = s * n + (d * H + h) * W + w;
                    out[i] = sg_edt_finish_value(grids + s * n, (int)D, (int)H, (int)W, (int)d, (int)h, (int)w, squared[i], level, value_scale,
                                                 keep_band);
                }
    return SG_OK;
}

}  // extern "C"
#pragma GCC pop_options
