/* l2q.h -- C ABI of libl2q.so: hand-written gfx950 (MI355X / CDNA4) kernels for the L2HMC /
 * HMC leapfrog integrator over 2D U(1) and 4D SU(3) lattice gauge fields.
 *
 * The reference (saforem2/l2hmc-qcd) is 100 % Python and has no FFI boundary; its hot path
 * is a sequence of ATen calls behind the Python classes `Dynamics`, `LatticeSU3`, `LatticeU1`,
 * `SU3`, `U1Phase`, `LeapfrogLayer`.  Each entry point below replaces one such ATen sequence;
 * the reference lines it replaces are cited (paths relative to src/l2hmc/ of the reference).
 * The Python classes of the same names in `l2hmc-qcd_amd/l2hmc/` call these through ctypes.
 *
 * Conventions
 *   - extern "C", plain C types.  All pointers are DEVICE pointers owned by the caller
 *     (normally PyTorch's allocator).  Nothing is allocated and nothing synchronises inside;
 *     work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - return 0 on success, negative L2Q_E* on failure; l2q_last_error() gives the text.
 *   - "native" SU(3) field layout (what every lattice kernel consumes and produces):
 *         xn[chain][mu][e][site]   complex128 (re, im interleaved, 16 B)
 *     with e = 3*row + col of the 3x3 link matrix and site = ((t*X + x)*Y + y)*Z + z.
 *     One wavefront reading entry e of 64 consecutive sites is a single coalesced 1 KiB load.
 *     The reference's public layout x[chain][mu][t][x][y][z][3][3] is converted at the API
 *     edge by l2q_su3_pack / l2q_su3_unpack; a trajectory stays in native layout throughout.
 *   - native flat index of a real per-entry quantity (masks, s/t/q network heads):
 *         j_n = (mu*9 + e)*V + site        (reference: j = (mu*V + site)*9 + e)
 *     native index of the 8-component algebra vector (vnet input):
 *         k_n = (mu*8 + a)*V + site        (reference: k = (mu*V + site)*8 + a)
 *   - U(1) fields keep the reference layout x[chain][2][T][X] (already site-contiguous).
 *   - per-chain reductions are order-stable (fixed tree, no atomics) so that dH and the
 *     accept/reject mask are reproducible run to run.
 */
#ifndef L2Q_H_
#define L2Q_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2Q_OK 0
#define L2Q_EINVAL (-1) /* bad argument (null pointer, non-positive size, bad enum) */
#define L2Q_ESHAPE (-2) /* inconsistent shapes / workspace too small */
#define L2Q_EHIP (-3)   /* HIP runtime error at launch */

/* activation enum for the network kernels (network/pytorch/network.py:40-46) */
#define L2Q_ACT_NONE 0
#define L2Q_ACT_TANH 1
#define L2Q_ACT_RELU 2
#define L2Q_ACT_LEAKY_RELU 3
#define L2Q_ACT_ELU 4
#define L2Q_ACT_SWISH 5

/* 16-bit operand types of l2q_gemm_h */
#define L2Q_HALF_F16 0
#define L2Q_HALF_BF16 1

const char* l2q_last_error(void);
int l2q_version(void);
/* performance knobs (results never depend on them), kept PER DEVICE: the call applies to the
 * calling thread's current HIP device -- the library's only state besides the last-error text
 * is this per-device table: "xcd_swizzle" in {0,1}; "force_tile" in {2,5,7} picks the SU(3) force
 * kernel design (5, the default: thread per link, su3_force_link.hip; 7: plaquettes shared between their
 * four links, su3_force_plaq.hip; 2: the slice-resident kernel of su3_force.hip, which otherwise runs only on lattices
 * too large for 5; su3_force.hip: pick_force decides).  Results agree to rounding across variants.  Returns the previous value, or L2Q_EINVAL for an unknown key/value.
 * (The Python binding applies L2Q_TUNING="key=value,..." from the environment when it loads the library.) */
int l2q_set_tuning(const char* key, int value);
/* Name (template instantiation as rocprofv3 prints it, without the l2q:: prefix) of the device
 * kernel that `entry` ("l2q_su3_force", "l2q_su3_force_kick", "l2q_su3_plaq_reduce", "l2q_su3_clover_reduce",
 * "l2q_su3_flow_stage": its launches joined by " + ", "l2q_vnet_heads_vupdate[_pair]_f64", "l2q_gemm_f64": kernel family only) dispatches
 * for a T x X x Y x Z lattice under the current tuning; "" for entry points with a single
 * kernel.  entry "l2q_gemm_h" with (T, X, Y) = (M, N, K): "hipblaslt" when that plain 16-bit layer goes to the
 * vendor library (gemm_lt.hip: library present, shape taken), "" when it runs on this build's kernels.  Lets a profile (rocprofv3 --pmc) be matched to the build that is running. */
int l2q_kernel_name(const char* entry, int T, int X, int Y, int Z, char* buf, size_t buf_bytes);
/* Select and check the device this process drives (one process per GPU): hipSetDevice(device),
 * refuses anything that is not gfx950, touches the device's knob table.  Returns `device` or a
 * negative error.  Optional -- every entry point works on the caller's current HIP device; this is
 * the explicit per-device handle SURVEY.md section 8(b)(ii) lists. */
int l2q_init(int device);

/* ---------------------------------------------------------------- the one collective of the path
 * Sum of the flat training-gradient buffer over ranks: the reference wraps the dynamics in
 * DistributedDataParallel (trainers/pytorch/trainer.py:246-257; bucketed all-reduce during
 * loss.backward(), :1296-1304) on the process group of utils/dist.py:126-144.  Thin wrapper over
 * RCCL (xGMI within a node); librccl is resolved at run time, so the library loads without it.
 * Bootstrap like NCCL: rank 0 calls l2q_comm_unique_id, the L2Q_COMM_ID_BYTES bytes reach the other
 * ranks out of band (a torch.distributed / file / env broadcast), every rank calls l2q_comm_init
 * with its HIP device current.  l2q_allreduce_grads is in place, enqueued on `stream`, elem_bytes
 * 8 = fp64, 4 = fp32 (one call per dtype group of the gradient arena).  Sampling never calls it. */
#define L2Q_COMM_ID_BYTES 128
int l2q_comm_unique_id(void* id_out);
int l2q_comm_init(const void* id, int nranks, int rank, void** comm_out);
int l2q_allreduce_grads(void* comm, void* grad, long n, int elem_bytes, void* stream);
int l2q_comm_destroy(void* comm);
/* teardown without a handshake with the peers (ncclCommAbort; falls back to destroy): for garbage collection
 * and interpreter shutdown, when the other ranks may be gone */
int l2q_comm_abort(void* comm);
/* version code of the RCCL library that was resolved (ncclGetVersion: major * 10000 + minor * 100 + patch), or a
 * negative error.  The wrapper declares the 2.x ABI by hand and refuses a library that reports another major. */
int l2q_comm_version(void);

/* bytes of scratch the reductions need for `nb` chains of `n_per_chain` work items */
size_t l2q_reduce_ws_bytes(int nb, long n_per_chain);

/* ---------------------------------------------------------------- layout conversion */
/* batched transpose in[batch][rows][cols] -> out[batch][cols][rows], elem_bytes in {4,8,16}.
 * pack:   reference [.., site, e] -> native [.., e, site]  (rows = V, cols = 9 or 8)
 * unpack: the same call with rows/cols swapped. */
int l2q_transpose(const void* in, void* out, long batch, int rows, int cols, int elem_bytes,
                  void* stream);
/* x[nb][4][V][3][3] c128 <-> xn[nb][4][9][V] c128 */
int l2q_su3_pack(const void* x_ref, void* x_nat, int nb, long V, void* stream);
int l2q_su3_unpack(const void* x_nat, void* x_ref, int nb, long V, void* stream);
/* x_ref[c] = unpack(mask[c] != 0 ? a_nat[c] : b_nat[c]): the accept / reject select of a transition
 * (x_out = ma x_prop + mr x_init, dynamics.py:677-682) fused into the native -> reference transpose of its
 * result; mask [nb] float32 (the acc_mask of l2q_accept) */
int l2q_su3_unpack_select(const void* a_nat, const void* b_nat, const float* mask, void* x_ref, int nb,
                          long V, void* stream);

/* ---------------------------------------------------------------- SU(3) lattice kernels */
/* Per-chain plaquette sums: out[c][0] = sum_{sites, 6 planes} Re tr P, out[c][1] = Im.
 * Replaces LatticeSU3._wilson_loops + the reductions in action/_plaquettes/_sin_charges/
 * _int_charges (lattice/su3/pytorch/lattice.py:157-269):
 *   action = -(beta/3) out[c][0];  plaqs = out[c][0]/(18 V);  sinQ = out[c][1]/(18 V);
 *   intQ = out[c][1]/(32 pi^2).   Algorithmic traffic: 576 B per (chain, site). */
int l2q_su3_plaq_reduce(const void* xn, int nb, int T, int X, int Y, int Z, double* out,
                        void* ws, size_t ws_bytes, void* stream);
/* The same sums kept per plane: out[c][p][0|1], p = 0..5 in the reference's order
 * (u,v) = (1,0),(2,0),(2,1),(3,0),(3,1),(3,2) -- what LatticeLoss._plaq_loss reduces to
 * (loss/pytorch/loss.py:57-70).  ws >= nb * ceil(V/256) * 12 doubles. */
int l2q_su3_plaq_planes(const void* xn, int nb, int T, int X, int Y, int Z, double* out, void* ws,
                        size_t ws_bytes, void* stream);
/* The trace field itself: out[p][c][site] = tr P_p(site), complex128, planes ordered as above -- the tensor
 * [6, nb, T, X, Y, Z] that LatticeSU3.wilson_loops returns (lattice/su3/pytorch/lattice.py:157-174, 242-244)
 * for callers that reduce it themselves (loss/pytorch/loss.py:57-110). */
int l2q_su3_wilson_loops(const void* xn, int nb, int T, int X, int Y, int Z, void* out, void* stream);
/* out[c] = sum_j (a[c][j] - b[c][j])^2 over n doubles (rmse loss, loss.py:131-148). */
int l2q_diff_norm2_reduce(const double* a, const double* b, int nb, long n, double* out, void* ws,
                          size_t ws_bytes, void* stream);
/* F = (beta/3) TAH(U_mu(x) * sum of 6 staples), written in native layout.
 * Replaces LatticeSU3.grad_action (autograd + projectTAH, lattice.py:299-308).
 * Algorithmic traffic: 1152 B per (chain, site). */
int l2q_su3_force(const void* xn, double beta, void* fn, int nb, int T, int X, int Y, int Z,
                  void* stream);
/* l2q_su3_force that also returns the plaquette sum of the x it was taken at: plaq[c] = sum over sites and the 6
 * planes of Re tr P (out[c][0] of l2q_su3_plaq_reduce, equal to rounding: another summation order; action =
 * -(beta/3) plaq[c]).  The thread-per-link kernel holds W = U A per link when it stores F, and sum_links Re tr W =
 * 4 sum_plaq Re tr P: it forms the real diagonal of W (which F does not need) and reduces it -- per thread over its
 * sweep, once over the workgroup, one partial per workgroup at a fixed index, then the fixed-order sum of
 * l2q_su3_plaq_reduce's second stage: no atomics, the same bits every run.  F is bit-identical to l2q_su3_force.  On
 * lattices (or under force_tile settings) that kernel does not serve, the ordinary force and the plaquette reduction
 * run one after the other.  ws: l2q_su3_force_action_ws_bytes(...) bytes. */
size_t l2q_su3_force_action_ws_bytes(int nb, int T, int X, int Y, int Z);
int l2q_su3_force_action(const void* xn, double beta, void* fn, double* plaq, int nb, int T, int X, int Y, int Z,
                         void* ws, size_t ws_bytes, void* stream);
/* The two calls above with an UPPER-PLANE output.  F is anti-Hermitian, plane (j, i) of a link is (-re, im) of plane
 * (i, j): fu [nb][4][6][V] holds planes e = 0, 4, 8 (the diagonal), 1, 2, 5 (i < j) of the native [nb][4][9][V]
 * field -- the same bits, signed zero on the real diagonal included -- and the other three are neither formed nor
 * stored (960 instead of 1152 B per (chain, site) with the read of x).  plaq keeps its bits.  An output form of the
 * thread-per-link kernel alone: L2Q_ESHAPE, nothing launched, where another force kernel serves the lattice (or
 * force_tile selects one) -- l2q_kernel_name answers "" there -- and the caller keeps the full field.  Consumers:
 * l2q_su3_projsu_digits_upper, l2q_vnet_heads_vupdate_sliced_upper_f64. */
int l2q_su3_force_upper(const void* xn, double beta, void* fu, int nb, int T, int X, int Y, int Z, void* stream);
int l2q_su3_force_action_upper(const void* xn, double beta, void* fu, double* plaq, int nb, int T, int X, int Y,
                               int Z, void* ws, size_t ws_bytes, void* stream);
/* fused plain-HMC half-kick: v += coef * F(x)  (dynamics/pytorch/dynamics.py:903-911,
 * coef = -eps/2); F is never materialised. */
int l2q_su3_force_kick(const void* xn, double beta, double coef, void* vn, int nb, int T,
                       int X, int Y, int Z, void* stream);
/* The same kick out of place: v_out = v_in + coef * (beta/3) TAH(U A)  (v_in == v_out is the call
 * above).  The first kick of a plain-HMC trajectory uses it to leave the momentum it was handed
 * untouched without copying it. */
int l2q_su3_force_kick_to(const void* xn, double beta, double coef, const void* v_in, void* v_out,
                          int nb, int T, int X, int Y, int Z, void* stream);
/* out = keep (.) x + expm(eps * v) @ ((1 - keep) (.) x), element-wise 0/1 mask on matrix
 * entries.  mask_n: float32 [36 V] in native order or NULL (keep = 0 everywhere: the plain
 * `update_gauge`, group/su3/pytorch/group.py:45-50).  keep = mask if !complement else 1-mask.
 * Replaces Dynamics._update_x_fwd/_bwd SU3 branch (dynamics.py:1420-1425, 1468-1474).
 * `out` may alias xn. */
int l2q_su3_expm_mul(const void* xn, const void* vn, double eps, const float* mask_n,
                     int complement, void* out, int nb, long V, void* stream);
/* Both half-updates of one leapfrog step in one pass (dynamics.py:1199-1203 forward:
 * keep = m then keep = 1-m; :1221-1225 backward: keep = 1-m then keep = m, i.e.
 * complement_first = 1), sharing one expm(eps v).  Equal to two l2q_su3_expm_mul calls up to
 * FMA contraction (1e-16).  `out` may alias xn. */
int l2q_su3_expm_mul2(const void* xn, const void* vn, double eps, const float* mask_n,
                      int complement_first, void* out, int nb, long V, void* stream);
/* l2q_su3_expm_mul2 that also writes vec[nb*4][8][V] = su3_to_vec(projectSU(x')) of the updated
 * links (group.py:138-147): the vnet input of the v-update that follows the x-update in a
 * leapfrog step (dynamics.py:1154-1156, 1204-1206), formed while x' is in registers. */
int l2q_su3_expm_mul2_vec8(const void* xn, const void* vn, double eps, const float* mask_n,
                           int complement_first, void* out, double* vec, int nb, long V,
                           void* stream);
/* l2q_su3_expm_mul2_vec8 / l2q_su3_projsu_vec8 that write the DIGITS of those values instead (the activation
 * digit image of l2q_gemm_digits_f64 below: row = chain, K = 32 V; image: l2q_gemm_digits_bytes(nb, 32 V) bytes,
 * 16-byte aligned; every value must satisfy |v| < 2^a_exp, else the next sliced layer's output is NaN).  Serve
 * V % 64 == 0 (and whole chains: nfields % 4 == 0), L2Q_EINVAL otherwise. */
int l2q_su3_expm_mul2_digits(const void* xn, const void* vn, double eps, const float* mask_n, int complement_first,
                             void* out, void* image, int a_exp, int nb, long V, void* stream);
int l2q_su3_projsu_digits(const void* in, void* image, int a_exp, long nfields, long V, void* stream);
/* l2q_su3_projsu_digits of an anti-Hermitian field given in upper-plane form, in[nfields][6][V]
 * (l2q_su3_force_upper): the three planes that are not stored are rebuilt in registers (a zero keeps the sign the
 * force kernel writes); the image bytes and the out-of-range flag are those of the full field. */
int l2q_su3_projsu_digits_upper(const void* in, void* image, int a_exp, long nfields, long V, void* stream);
/* l2q_su3_pack and l2q_su3_projsu_digits of its result from ONE read of the reference-layout field (a
 * trajectory's entry): x_nat has the bits of l2q_su3_pack(x_ref), image the bytes of
 * l2q_su3_projsu_digits(x_nat, nb * 4 fields).  V % 64 == 0 and 16-byte aligned pointers, as there. */
int l2q_su3_pack_digits(const void* x_ref, void* x_nat, void* image, int a_exp, int nb, long V, void* stream);
/* projectSU on every link (group/su3/pytorch/utils.py:341-346); out may alias in. */
int l2q_su3_project_su(const void* in, void* out, long nfields, long V, void* stream);
/* su3_to_vec(projectSU(.)) -> vec[nfields][8][V] double (group.py:138-147); the vnet
 * GEMM A-operand (dynamics.py:1154-1156). */
int l2q_su3_projsu_vec8(const void* in, double* vec, long nfields, long V, void* stream);
/* projectU: x (x^H x)^(-1/2) without the determinant phase (utils.py:332-338). */
int l2q_su3_project_u(const void* in, void* out, long nfields, long V, void* stream);
/* out = op(a) op(b) per link, op = adjoint if flagged (SU3.mul, group.py:56-69). */
int l2q_su3_mul(const void* a, const void* b, int adjoint_a, int adjoint_b, void* out,
                long nfields, long V, void* stream);
/* projectTAH on every link (group.py:92-103); out may alias in. */
int l2q_su3_project_tah(const void* in, void* out, long nfields, long V, void* stream);
/* out[c] = 0.5 * sum_links (|p|_F^2 - 8)   (group.py:125-126) */
int l2q_su3_kinetic_reduce(const void* vn, int nb, long V, double* out, void* ws,
                           size_t ws_bytes, void* stream);
/* momenta from 8 standard-normal fields normals[8][nfields*V] in the reference's draw order
 * r3, r8, r01, r02, r12, i01, i02, i12 (group/su3/pytorch/utils.py:171-195). */
int l2q_su3_assemble_tah(const double* normals, void* vn, long nfields, long V, void* stream);
/* The same for whole chains (4 nb fields) with norm2[c] = sum over the chain's 36 V entries of |p|^2, summed
 * from the values as stored (fixed order; l2q_su3_kinetic_reduce of vn is 0.5 * (norm2[c] - 32 V) to rounding).
 * ws >= nb * 4 * ceil(V/256) doubles. */
int l2q_su3_assemble_tah_norm2(const double* normals, void* vn, int nb, long V, double* norm2, void* ws,
                               size_t ws_bytes, void* stream);
/* max over links of |x^H x - 1|_F^2 + |det x - 1|^2 and its mean, per chain
 * (checkSU, utils.py:376-391): out[c][0] = sqrt(mean/20), out[c][1] = sqrt(max/20). */
int l2q_su3_check_su(const void* xn, int nb, long V, double* out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---------------------------------------------------------------- Wilson flow and clover observables */
/* Clover sums per chain, raw (before 1/V and 1/4 pi^2): with F_{mu nu}(x) = TAH(Q_{mu nu}(x)) / 4, Q_{mu nu} the sum
 * of the four counter-clockwise plaquette leaves of the (mu, nu) plane that start and end at x,
 *   out[c][0] = sum_x sum_{mu<nu} -tr F_{mu nu} F_{mu nu}            (E = out[c][0] / V >= 0)
 *   out[c][1] = sum_x -tr(F01 F23 - F02 F13 + F03 F12)               (Q = out[c][1] / (4 pi^2))
 *   out[c][2] = sum_x sum_{mu<nu} Re tr P_{mu nu}(x)                 (= out[c][0] of l2q_su3_plaq_reduce)
 * Anchor of sign and normalisation: uniform abelian fluxes n01, n23 along diag(1, -1, 0) give
 * Q = 2 n01 n23 (sin phi01 / phi01)(sin phi23 / phi23), E = 2 (sin^2 phi01 + sin^2 phi23).
 * Takes any lattice (extents 1 and 2 included); where X Y Z is whole 64-site tiles (8^4, 16^4) a slice-resident
 * kernel keeps three time slices of a tile in LDS.  ws as for l2q_su3_plaq_reduce.  Algorithmic traffic: 576 B
 * per (chain, site). */
int l2q_su3_clover_reduce(const void* xn, int nb, int T, int X, int Y, int Z, double* out,
                          void* ws, size_t ws_bytes, void* stream);
/* One low-storage stage of the Wilson flow (always the plaquette action):
 *   P_out = P_in + c * TAH(U A)  (A = the 6 staples of l2q_su3_force; p_in NULL = 0),   X_out = exp(s * P_out) X_in
 * on all links, out of place: x_out != x_in, p_out is required and may alias p_in.  Two launches (the force kick
 * at beta = 3 into p_out, then the unmasked l2q_su3_expm_mul) on every lattice. */
int l2q_su3_flow_stage(const void* x_in, const void* p_in, double c, double s, void* p_out, void* x_out,
                       int nb, int T, int X, int Y, int Z, void* stream);
/* One third-order step of size eps of dV/dt = Z(V) V, Z = -TAH(V A) (Luescher, arXiv:1006.4518):
 * three stages with (P_in, c, s) = (0, 1, -eps/4), (P, -32/17, 17 eps/36), (P, 27/17, -17 eps/36), the links
 * going x_in -> x_out -> ws_x -> x_out.  x_in is only read; ws_p and ws_x are scratch fields of the links' size;
 * x_in, x_out, ws_x must be three different fields. */
int l2q_su3_flow_step(const void* x_in, void* x_out, void* ws_p, void* ws_x, double eps, int nb, int T, int X,
                      int Y, int Z, void* stream);
/* The same step with an embedded error estimate for a step-size controller (csrc/su3_flow_adaptive.hip; Fritzsch &
 * Ramos, arXiv:1301.4388 App. D).  With G_i = TAH(W_i A(W_i)), Z_i = -eps G_i and the low-storage generators kept
 * apart, P1 = G0, P2 = P1 - 32/17 G1, P3 = P2 + 27/17 G2 (as l2q_su3_flow_step_bwd keeps them),
 *   W3 = exp(-17 eps/36 P3) W2  -> x_out                                  (third order, the step of l2q_su3_flow_step)
 *   W' = exp(-Z0 + 2 Z1) W0 = exp(eps/16 (17 P2 - P1)) W0                 (second order, never stored)
 *   d[c] = max over mu, x of |W3 - W'|_F / 9                              (9 = N^2), an O(eps^3) quantity
 * Stages 1 and 2 are l2q_su3_flow_stage, stage 3 the force kick into P3 and ONE kernel, thread per link, that reads
 * W0, W2, P1, P2, P3, forms both products in registers, writes W3 and reduces d: 864 B per link (two
 * l2q_su3_expm_mul and a distance pass move 1296 B).  A link whose distance is not finite makes d[c] = +inf.  The
 * operations on a link depend on the link only: a chain's x_out and d[c] are the same bits alone and in a batch; x_out
 * differs from l2q_su3_flow_step's only by the FMA contraction of the kernel hosting the last product (1e-16).
 * x_in is only read, so a rejected step is retried from it.  ws_p3 is THREE consecutive fields of the links' size
 * (P1, P2, P3), ws_x one; x_in, x_out, ws_x must be three different fields outside ws_p3 (L2Q_EINVAL).  With the
 * caller's two ping-pong fields that is six fields beside the input.  ws >= l2q_su3_flow_step_err_ws_bytes
 * (one double per 256 links; L2Q_ESHAPE). */
size_t l2q_su3_flow_step_err_ws_bytes(int nb, int T, int X, int Y, int Z);
int l2q_su3_flow_step_err(const void* x_in, void* x_out, void* ws_p3 /* three fields */, void* ws_x, double eps,
                          double* d /* [nb] */, int nb, int T, int X, int Y, int Z,
                          void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- Wilson loops R x T and Polyakov loops */
/* A line is L_mu(x, n) = U_mu(x) U_mu(x + mu) ... U_mu(x + (n-1) mu), periodic; a field of lines has the shape and the
 * native layout xn[chain][mu][e][site] of a link field, and L(., 1) is the links.  One more link on every line:
 *   lines_out_mu(x) = lines_in_mu(x) U_mu(x + n mu)      for all four mu, n >= 0 taken modulo the extent
 * (n = the length of the lines in lines_in makes them one longer).  lines_out may alias lines_in: each site reads and
 * writes only its own entry of it.  lines_out must not alias xn, which is read at another site.  Replaces a
 * torch.roll of the unpacked links and a batched 3x3 matmul per link added.  Streaming; algorithmic traffic:
 * 3 x 576 B per (chain, site). */
int l2q_su3_line_extend(const void* lines_in, const void* xn, int n, void* lines_out, int nb, int T, int X, int Y,
                        int Z, void* stream);
/* Sums of planar loops closed from two line fields, a of length r and b of length t (r, t >= 1): for the 12 ordered
 * pairs mu != nu, in the plaquette convention P_{mu nu}(x) = U_mu(x) U_nu(x+mu) U_mu(x+nu)^H U_nu(x)^H,
 *   W_{mu nu}(x) = a_mu(x) b_nu(x + r mu) a_mu(x + t nu)^H b_nu(x)^H
 *   out[c][k][0|1] = sum_x Re | Im tr W_{mu nu}(x),      k = 3 mu + (nu < mu ? nu : nu - 1)
 * a = b = the links with r = t = 1 gives the plaquette sums: pairs mu > nu are the planes of l2q_su3_plaq_planes,
 * pairs mu < nu their conjugates.  The shifts are taken modulo the extents, so r or t equal to or beyond an extent
 * is legal and wraps; any lattice (extents 1 and 2 included); a and b may be the same field.  Two-stage reduction as
 * l2q_su3_plaq_planes: ws >= nb * ceil(V/256) * 24 doubles (6 x l2q_reduce_ws_bytes(nb, V) covers it).  Replaces, per
 * (r, t), four torch.roll and three batched 3x3 matmuls over the unpacked fields for each of the 12 pairs.
 * Algorithmic traffic: 2 x 576 B per (chain, site) (a and b once each; the shifted operands are re-reads). */
int l2q_su3_loop_reduce(const void* a, int r, const void* b, int t, double* out, int nb, int T, int X, int Y, int Z,
                        void* ws, size_t ws_bytes, void* stream);
/* Polyakov loops in direction mu (0..3): out[c][x_perp] = tr prod_{k < N_mu} U_mu(x_perp, x_mu = k), complex128, not
 * divided by 3; the perpendicular sites are in the lattice's own order with direction mu removed ([nb][X][Y][Z] for
 * mu = 0).  Extent 1 gives tr U.  Replaces N_mu - 1 batched matmuls over slices of the unpacked links.  Algorithmic
 * traffic: 144 B per (chain, site) read, 16 B per (chain, perpendicular site) written. */
int l2q_su3_polyakov(const void* xn, int mu, void* out, int nb, int T, int X, int Y, int Z, void* stream);

/* ---------------------------------------------------------------- SU(3) heatbath and overrelaxation */
/* Local updates of the Wilson action (c1 = 0), IN PLACE: both rewrite the links U_mu(x) of every chain at the sites
 * with (t + x + y + z) & 1 == parity and only read every other link.  All four extents must be even (L2Q_ESHAPE
 * otherwise): the staples of U_mu(x) then hold mu-links of the other parity only, so no thread of a launch reads what
 * another one writes.  One thread per (chain, half-site h); h runs over the sites of that parity in lattice order,
 * s = 2 h + ((parity - t - x - y) & 1).
 * With A = A_mu(x) the sum of the six staples as in l2q_su3_force (the link's share of the action is
 * -(beta/3) Re tr(U A)), for the SU(2) subgroups (i, j) = (0,1), (0,2), (1,2) in that order, W = U A formed anew:
 *   r = (Re(W_ii + W_jj), Im(W_ij + W_ji), Re(W_ij - W_ji), Im(W_ii - W_jj)) / 2, k = |r|, rh = r / k  ((1,0,0,0) if
 *   k is zero or not finite); a quaternion a is the block [[a0 + i a3, a2 + i a1], [-a2 + i a1, a0 - i a3]] at rows and
 *   columns i, j, and U <- embed(a) U with
 *   overrelaxation: a = conj(rh) conj(rh)  (Re tr(U A) unchanged);
 *   heatbath (Cabibbo-Marinari with Kennedy-Pendleton sampling): alpha = 2 beta k / 3, v = 1 - u; tries t = 0..ntry-1:
 *     delta = -(ln v1 + cos^2(2 pi v2) ln v3) / alpha, the first with v4^2 <= 1 - delta/2 gives b0 = 1 - delta;
 *     cos(theta) = 1 - 2 v5, phi = 2 pi v6, n = sqrt(max(0, 1 - b0^2)),
 *     b = (b0, n sin(theta) cos(phi), n sin(theta) sin(phi), n cos(theta)), a = b conj(rh).
 *     No try accepted: the subgroup leaves U as it is and counts one failure (still exact: whether that happens
 *     depends on the staples only).
 * u[nb][3][4 ntry + 2][V/2] float64 uniforms in [0, 1), half-site fastest: rows 4t .. 4t+3 are u1..u4 of try t, the
 * last two rows u5, u6; ntry in 1..16.  The kernel holds no generator.  fails (may be NULL) [nb]: the (link, subgroup)
 * failures of each chain in this launch, by block partials in ws >= nb * ceil(V/2 / 256) doubles
 * (l2q_reduce_ws_bytes(nb, V/2) covers it); with fails NULL, ws is not used.
 * Algorithmic traffic per updated link: 20 x 144 B of links (18 staple links, the link read and written) plus
 * 24 (4 ntry + 2) B of uniforms. */
int l2q_su3_heatbath(void* xn, double beta, int mu, int parity, const double* u, int ntry, double* fails, int nb,
                     int T, int X, int Y, int Z, void* ws, size_t ws_bytes, void* stream);
int l2q_su3_overrelax(void* xn, int mu, int parity, int nb, int T, int X, int Y, int Z, void* stream);

/* ---------------------------------------------------------------- SU(3) Landau and Coulomb gauge fixing */
/* Gauge directions D: a 4-bit set `dirmask` (bit mu = direction mu) in 1..15 with at least two bits set; Landau gauge is
 * 15, Coulomb gauge with time direction t is 15 & ~(1 << t).  A gauge transformation acts in all four directions
 * whatever D is: U_mu(x) -> g(x) U_mu(x) g(x+mu)^H.  Per chain:
 *   functional (maximised)  F = (1 / (3 |D| V)) sum_x sum_{mu in D} Re tr U_mu(x)
 *   residual                theta = (1 / (3 V)) sum_x tr Delta(x) Delta(x)^H,
 *                           Delta(x) = sum_{mu in D} [A_mu(x) - A_mu(x-mu)],  A_mu(x) = (U - U^H) / (2i) - tr(.) / 3
 * (conventions of Giusti et al., hep-lat/0104012).
 * Local step at a site x (Los Alamos iteration with overrelaxation; SU(3) through the SU(2) subgroups and the
 * quaternion / embed conventions of the heatbath above):  K(x) = sum_{mu in D} [U_mu(x) + U_mu(x-mu)^H], g = 1, W = K;
 * for (i, j) = (0,1), (0,2), (1,2): r from W as above, k = |r|, rh = r / k; k zero or not finite: the subgroup step
 * is the identity; else a = conj(rh) = (cos phi, n sin phi) with phi = atan2(|a_vec|, a0) in [0, pi], the step is the
 * exact power a^omega = (cos(omega phi), n sin(omega phi)) (a_vec = 0: the identity), g <- embed(a^omega) g,
 * W <- embed(a^omega) W.  Then for all four mu: U_mu(x) <- g U_mu(x), U_mu(x-mu) <- U_mu(x-mu) g^H.  For omega in
 * [1, 2) every subgroup step has Re tr(a^omega W) >= Re tr W: F cannot decrease.
 * l2q_su3_gaugefix_sweep does that step, IN PLACE, at the sites with (t + x + y + z) & 1 == parity (half-site order as
 * the heatbath).  All four extents must be even (L2Q_ESHAPE): each link then has one end on each parity, so one launch
 * rewrites every link of the field exactly once and reads only links that the same thread rewrites -- also at extent
 * 2, where x+mu and x-mu are one site but U_mu(x) and U_mu(x-mu) two links.  One sweep is parity 0, then parity 1.
 * gn (may be NULL): the accumulated transformation G[nb][9][V] complex128, one matrix per site, component-major as a
 * link; with it G(x) <- g G(x).  active (may be NULL): int32 [nb] on the device; a chain with active[c] == 0 is not
 * touched at all.  omega must be finite and in [1, 2) (L2Q_EINVAL).  Algorithmic traffic per launch: the field read
 * and written once (8 links x 144 B each way per half-site), 144 B each way more with gn. */
int l2q_su3_gaugefix_sweep(void* xn, void* gn, const int* active, int dirmask, int parity, double omega, int nb,
                           int T, int X, int Y, int Z, void* stream);
/* out[nb][2] = (F, theta) of each chain, any extents.  Two-stage reduction in a fixed order: ws >= nb * ceil(V/256) * 2
 * doubles (l2q_reduce_ws_bytes(nb, V) covers it; L2Q_ESHAPE).  A chain's values do not depend on the batch. */
int l2q_su3_gauge_condition(const void* xn, int dirmask, double* out, int nb, int T, int X, int Y, int Z, void* ws,
                            size_t ws_bytes, void* stream);
/* out_mu(x) = G(x) U_mu(x) G(x+mu)^H for all four mu, gn = G[nb][9][V] as above; any extents; out must alias neither
 * xn nor gn (L2Q_EINVAL). */
int l2q_su3_gauge_apply(const void* xn, const void* gn, void* out, int nb, int T, int X, int Y, int Z, void* stream);

/* ---------------------------------------------------------------- SU(3) APE and HYP link smearing */
/* csrc/su3_smear.hip.  For a side field A (links of direction nu) and a forward field B (links of direction mu) the two
 * staples of direction nu around a mu-link, in the plaquette convention of l2q_su3_force, are
 *   S_nu[A, B](x) = A(x) B(x+nu) A(x+mu)^H  +  A(x-nu)^H B(x-nu) A(x-nu+mu).
 * Proj is the projection of l2q_su3_project_su: the unitary (polar) factor X (X^H X)^(-1/2) with the phase of its
 * determinant divided out -- not the iterative maximisation of Re tr(V X^H) that some codes use.  It is accurate while
 * the matrix it is given stays well conditioned (condition number up to ~100: fields near the unit circle).
 * All four entry points are out of place and take any extents (odd, 1 and 2 as well): nothing is updated in place, so
 * the checkerboard kernels' even-extent rule does not apply.  L2Q_EINVAL, before any HIP call: a null pointer; an
 * output that aliases an input; a non-positive size or a chain of more than 2^31 / 36 sites; alpha not finite or
 * outside [0, 1]; for APE a dirmask outside 1..15 or with fewer than two bits set.  One thread per (chain, output field, site); a chain's result does not depend
 * on the batch.
 * APE step with the directions D = dirmask (bit mu = direction mu), n = |D| - 1:
 *   mu in D:      out_mu = Proj[(1 - alpha) U_mu + (alpha / 2n) sum_{nu in D, nu != mu} S_nu[U_nu, U_mu]]
 *   mu not in D:  out_mu = U_mu, copied bit for bit; such links enter no staple.
 * dirmask 15 is the 4D step; 15 & ~(1 << t) smears the three directions of the slices of direction t within each slice.
 * Algorithmic traffic: 1152 B per (chain, site), the field read and written once. */
int l2q_su3_ape_smear(const void* xn, double alpha, int dirmask, void* out, int nb, int T, int X, int Y, int Z,
                      void* stream);
/* HYP smearing (Hasenfratz & Knechtli) in three levels, each projected; eta = 6 - mu - nu - rho, the fourth direction:
 *   level 1:  B1[mu][eta] = Proj[(1 - alpha3) U_mu + (alpha3 / 2) S_eta[U_eta, U_mu]]          (V-bar_{mu; nu rho})
 *   level 2:  B2[mu][nu]  = Proj[(1 - alpha2) U_mu + (alpha2 / 4) sum_{rho != mu, nu} S_rho[B1[rho][eta], B1[mu][eta]]]
 *   level 3:  V_mu        = Proj[(1 - alpha1) U_mu + (alpha1 / 6) sum_{nu != mu} S_nu[B2[nu][mu], B2[mu][nu]]]
 * b1 and b2 are decorated fields: the 12 fields F[mu][o], o != mu, of a level in the native layout [nb][4][3][9][V],
 * index order mu, then k with o = k + (k >= mu) (the pair order of l2q_su3_loop_reduce), then entry, then site: three link
 * fields in size (432 B per (chain, site)).  Algorithmic traffic per (chain, site): level 1 2304 B (links read, b1
 * written), level 2 4032 B (links and b1 read, b2 written), level 3 2880 B (links and b2 read, links written). */
int l2q_su3_hyp_level1(const void* xn, double alpha3, void* b1, int nb, int T, int X, int Y, int Z, void* stream);
int l2q_su3_hyp_level2(const void* xn, const void* b1, double alpha2, void* b2, int nb, int T, int X, int Y, int Z,
                       void* stream);
int l2q_su3_hyp_level3(const void* xn, const void* b2, double alpha1, void* out, int nb, int T, int X, int Y, int Z,
                       void* stream);

/* ---------------------------------------------------------------- SU(3) Wilson fermions */
/* csrc/su3_wilson.hip.  Spinor fields are psi[nb][nrhs][12][V] complex128, component 3 spin + colour, the site index of
 * the links; a system is one (chain, rhs) pair.  The Wilson-Dirac operator on the links xn (thin or smeared):
 *   M psi = psi - kappa H psi,
 *   H psi(x) = sum_mu [(1 - gamma_mu) U_mu(x) psi(x+mu) + (1 + gamma_mu) U_mu(x-mu)^H psi(x-mu)].
 * Gamma matrices: Hermitian, chiral, gamma_mu = [[0, B_mu], [B_mu^H, 0]] in 2 x 2 blocks with B_0 = 1 (direction 0 is T)
 * and B_k = -i sigma_k for k = 1, 2, 3 (x, y, z); gamma5 = gamma_0 gamma_1 gamma_2 gamma_3 = diag(-1, -1, 1, 1).
 * flags bit 0 (dagger): M^H = gamma5 M gamma5, the two projector signs swapped.  flags bit 1: antiperiodic in direction
 * 0, every hop across the t = T-1 -> 0 seam, either way, takes a factor -1; otherwise periodic.  Any extents: with an
 * extent of 1 or 2 the forward and the backward neighbour coincide and both terms are added (T = 1: both carry the sign).
 * H does not depend on the gauge action.  Out of place.  One thread per (system, site), 1320 flops; algorithmic traffic
 * per (system, site) 384 B of spinors (read once, written once; the eight neighbours come from cache) and 576 B of
 * links, which the nrhs systems of a chain share.
 * norm_part (may be null): [nb][nrhs][parts] partial sums of |out|^2, one per workgroup, parts =
 * l2q_su3_wilson_norm_parts(T, X, Y, Z) = ceil(V / 256) (0 for extents the kernels refuse).  A workgroup belongs to one
 * system and sums in a fixed order: a system's partials are the same bits whatever else the batch holds.
 * L2Q_EINVAL, before any HIP call: a null xn, psi or out; out aliasing psi (or xn); a non-positive size; nb * nrhs *
 * 12 * V of 2^31 or more; kappa not finite; flags outside 0..3. */
long l2q_su3_wilson_norm_parts(int T, int X, int Y, int Z);
int l2q_su3_wilson_apply(const void* xn, const void* psi, void* out, double* norm_part, double kappa, int flags, int nb,
                         int nrhs, int T, int X, int Y, int Z, void* stream);
/* One pass of a CG iteration over nsys systems of V sites: x += alpha[s] p, r -= alpha[s] q, and rr_part[nsys][ceil(V /
 * 256)] = partial sums of |r|^2 of the new r, in the fixed order of the apply's.  alpha is a device array [nsys] of
 * doubles.  alpha[s] = 0 leaves x and r of that system the same bits.  L2Q_EINVAL: a null pointer; x or r aliasing
 * another field; a non-positive size or nsys * 12 * V of 2^31 or more. */
int l2q_su3_spinor_cg_update(void* x, void* r, const void* p, const void* q, const double* alpha, double* rr_part,
                             long nsys, long V, void* stream);
/* p = z + beta[s] p, beta a device array [nsys] of doubles.  L2Q_EINVAL as above (p must not alias z). */
int l2q_su3_spinor_xpay(void* p, const void* z, const double* beta, long nsys, long V, void* stream);
/* csrc/su3_spinor_mshift.hip: the BLAS-1 kernels of multi-shift CG (Jegerlehner, hep-lat/9612014).  Shifted fields are
 * f[nsys][ns][12][V] complex128, contiguous: a (system, shift) pair is a system of every other spinor entry, so the same
 * memory read as [nsys * ns][12][V] feeds the operator, the hops and the force.  r, p, z and out are [nsys][12][V]; V is
 * the site count of the fields, a half lattice included.  Coefficients are device arrays of doubles.
 * l2q_su3_spinor_mshift_update, the fused step of an iteration, per system s, with the new residual r:
 *   p <- r + beta[s] p;  for every shift k with live[s][k] != 0:  x_k += a[s][k] p_k, then p_k <- zeta[s][k] r + b[s][k] p_k
 * (the old p_k in the first).  a, b, zeta: [nsys][ns]; beta: [nsys]; live: [nsys][ns] int32.  A shift that is not live is
 * neither read nor written: its x_k and p_k keep their bits.  r is read once: 3 + 4 (live shifts) field streams per site.
 * L2Q_EINVAL, before any HIP call: a null pointer; r, p, x or ps overlapping one another (as byte ranges, so r aliasing
 * any x_k or p_k is caught); ns < 1; a non-positive size or nsys * ns * 12 * V of 2^31 or more. */
int l2q_su3_spinor_mshift_update(void* x, void* ps, void* p, const void* r, const double* a, const double* b,
                                 const double* zeta, const double* beta, const int* live, long nsys, long ns, long V,
                                 void* stream);
/* The residual step: r -= alpha[s] z, and rr_part[nsys][ceil(V / 256)] = partial sums of |r|^2 of the new r, in the fixed
 * order of l2q_su3_spinor_cg_update.  L2Q_EINVAL: a null pointer; r aliasing z; a bad size as there. */
int l2q_su3_spinor_axmy_norm(void* r, const void* z, const double* alpha, double* rr_part, long nsys, long V,
                             void* stream);
/* out[s] = sum_k w[s][k] x[s][k] over the ns fields of a system, summed in the order of k; w: [nsys][ns].  L2Q_EINVAL: a
 * null pointer; out overlapping x; ns < 1; a bad size as for l2q_su3_spinor_mshift_update. */
int l2q_su3_spinor_lincomb(const void* x, const double* w, void* out, long nsys, long ns, long V, void* stream);
/* csrc/su3_wilson_force.hip.  The force of npf two-flavour pseudofermion fields, S_f = sum_r phi_r^H (M^H M)^-1 phi_r,
 * from the solutions X_r = (M^H M)^-1 phi_r and Y_r = M X_r, both [nb][npf][12][V]: the TAH field F_f with dS_f/dt =
 * sum_links <p, F_f>, <a, b> = Re tr(a^H b), under dU/dt = p U (the convention of l2q_su3_force).  With s the seam sign
 * of l2q_su3_wilson_apply (-1 on a hop across t = T-1 -> 0 with flags bit 1, mu = 0; else +1), X' = s X(x+mu), Y' =
 * s Y(x+mu) and a b^H the colour outer product summed over spin, (a b^H)_ij = sum_spin a_(spin,i) conj(b_(spin,j)):
 *   W_mu(x) = U_mu(x) sum_r [(1 - gamma_mu) X'_r] Y_r(x)^H - sum_r X_r(x) [(1 + gamma_mu) Y'_r]^H U_mu(x)^H,
 *   F_f,mu(x) = -2 kappa TAH(W_mu(x)),   TAH(W) = (W - W^H)/2 - (tr/3) 1.
 * f_out = (f_in ? f_in : 0) + coef F_f in the native link layout [nb][4][9][V]: coef = 1 with f_in = NULL is the force,
 * f_in == f_out = v with coef = -eps/2 the in-place kick (as l2q_su3_force_kick), another f_in the kick out of place (as
 * l2q_su3_force_kick_to).  flags bit 1: antiperiodic in t, the bit of l2q_su3_wilson_apply; no other bit.  Any extents,
 * 1 and 2 included (T = 1: every hop in t carries the sign).  One thread per link, no atomics, the sum over r in its
 * order: a chain's force is the same bits alone and in a batch, and from run to run.  F_f is stored exactly
 * anti-Hermitian: plane (j, i) is (-re, im) of plane (i, j), the diagonal has no real part (with f_in: if f_in is).
 * Algorithmic traffic per (chain, site): links 576 B, output 576 B (+ 576 B of f_in), spinors npf * 384 B.
 * L2Q_EINVAL, before any HIP call: a null xn, X, Y or f_out; f_out aliasing xn, X or Y; kappa or coef not finite;
 * npf <= 0 or another non-positive size; nb * npf * 12 * V of 2^31 or more; flags other than 0 or 2. */
int l2q_su3_wilson_force(const void* xn, const void* X, const void* Y, const void* f_in, void* f_out, double kappa,
                         double coef, int flags, int nb, int npf, int T, int X_, int Y_, int Z, void* stream);
/* csrc/su3_wilson_eo.hip.  The half-lattice hop of even-odd preconditioning.  H couples sites of opposite parity only
 * (parity of a site: (t + x + y + z) & 1, 0 even), so M psi = b reduces to the Schur system on the even sites,
 *   Mhat psi_e = b_e + kappa H_eo b_o,   Mhat = 1 - kappa^2 H_eo H_oe,   psi_o = b_o + kappa H_oe psi_e.
 * A half field is psi_h[nb][nrhs][12][V/2] complex128: the sites of one parity in lexicographic order; with Z even the
 * sites 2h and 2h + 1 have opposite parity, so site s of either parity has the half index s >> 1.  The links xn stay in
 * the full native layout [nb][4][9][V].  For every system and every site x of parity `parity`:
 *   out(x) = b aux(x) + a (H src)(x),
 * src a half field on the other parity, aux and out half fields on `parity`; aux may be null, then the b term is absent.
 * H, the gamma basis, the seam sign and flags (bit 0 dagger: the projector signs swapped, gamma5 H gamma5; bit 1
 * antiperiodic in t) are those of l2q_su3_wilson_apply; the dagger bit on both hops gives Mhat^H.  Uses: H_oe or H_eo
 * alone (a = 1, b = 0, aux null); the second half of Mhat (a = -kappa^2, b = 1, aux = psi_e); the source b_e + kappa
 * H_eo b_o and the reconstruction b_o + kappa H_oe psi_e (a = kappa, b = 1).  All four extents even; an extent of 2 is
 * legal: the forward and the backward neighbour coincide and both terms are added.  out may be aux; it must not be src
 * or xn.  One thread per (system, half-site), 1320 flops (+ 48 with aux); algorithmic traffic per (system, half-site)
 * 192 B of output, 192 B of aux if given, 192 B of src (each entry read once; the eight neighbours come from cache) and
 * 1152 B of links, the eight links at and behind the site, which the nrhs systems of a chain share -- each link load
 * reads every second site of a link plane and so uses half of every cache line it touches.
 * norm_part (may be null): [nb][nrhs][ceil((V/2) / 256)] partial sums of |out|^2, one per workgroup, in the fixed order
 * of l2q_su3_wilson_apply's: a system's partials are the same bits whatever else the batch holds.
 * L2Q_EINVAL, before any HIP call: a null xn, src or out; out aliasing src or xn; a non-positive size; nb * nrhs * 12 *
 * V of 2^31 or more; a or b not finite; flags outside 0..3; parity not 0 or 1.  L2Q_ESHAPE: an odd extent. */
int l2q_su3_wilson_hop_eo(const void* xn, const void* src, const void* aux, void* out, double* norm_part, double a,
                          double b, int flags, int parity, int nb, int nrhs, int T, int X, int Y, int Z, void* stream);
/* csrc/su3_wilson_f32.hip.  The single-precision kernels of the mixed-precision even-odd solves (defect correction: the
 * inner CG on Mhat runs on these, the outer loop recomputes the true residual with the fp64 entries above).
 * l2q_su3_links_demote_eo: the fp32, parity-ordered copy of the native links xn[nb][4][9][V] complex128,
 *   x32[nb][parity][4][9][V/2] float2: entry h of parity p is the link at the site of parity p of the pair (2h, 2h + 1),
 * every entry rounded to float once.  One thread per (chain, half-site), plain vector loads and stores.  L2Q_EINVAL: a
 * null pointer; x32 aliasing xn; a non-positive size.  L2Q_ESHAPE: an odd extent. */
int l2q_su3_links_demote_eo(const void* xn, void* x32, int nb, int T, int X, int Y, int Z, void* stream);
/* out = b aux + a H src on the sites of `parity`: l2q_su3_wilson_hop_eo on float2 half fields [nb][nrhs][12][V/2] and the
 * link copy x32 of l2q_su3_links_demote_eo, with its semantics and argument checks (aux and norm_part may be null, out
 * may be aux, an extent of 2 is legal; the same gamma basis, seam sign and flags).  The forward link of a site is entry h
 * of this parity's block of x32, the backward link entry s' >> 1 of the other parity's: every link load is contiguous
 * across lanes.  Arithmetic in float (a and b are rounded to float); one thread per (system, half-site), 8 B per lane
 * and plane; algorithmic traffic per (system, half-site) 96 B of output, 96 B of aux if given, 96 B of src and 576 B of
 * links, which the nrhs systems of a chain share.  norm_part: [nb][nrhs][ceil((V/2) / 256)] doubles; every thread adds
 * its 24 squares in double and the block partial is the fixed tree of the fp64 kernels: a system's partials are the same
 * bits whatever else the batch holds.  Errors as l2q_su3_wilson_hop_eo. */
int l2q_su3_wilson_hop_eo_f32(const void* x32, const void* src, const void* aux, void* out, double* norm_part, double a,
                              double b, int flags, int parity, int nb, int nrhs, int T, int X, int Y, int Z,
                              void* stream);
/* l2q_su3_spinor_cg_update and l2q_su3_spinor_xpay on float2 fields: alpha and beta stay device arrays [nsys] of doubles
 * and are rounded to float in the kernel; rr_part stays double, every thread adding its squares in double.  Errors as
 * there. */
int l2q_su3_spinor_cg_update_f32(void* x, void* r, const void* p, const void* q, const double* alpha, double* rr_part,
                                 long nsys, long V, void* stream);
int l2q_su3_spinor_xpay_f32(void* p, const void* z, const double* beta, long nsys, long V, void* stream);
/* out32 = scale[s] in64: nsys systems of 12 V entries, complex128 to float2, scale a device array [nsys] of doubles; the
 * product in double, rounded to float once.  L2Q_EINVAL: a null pointer; out32 aliasing in64; a size as above. */
int l2q_su3_spinor_demote(const void* in64, const double* scale, void* out32, long nsys, long V, void* stream);
/* x64 += scale[s] e32, product and sum in double; a system with scale[s] = 0 is not written and keeps its bits.
 * L2Q_EINVAL: a null pointer; x64 aliasing e32; a size as above. */
int l2q_su3_spinor_promote_axpy(void* x64, const void* e32, const double* scale, long nsys, long V, void* stream);
/* csrc/su3_wilson_clover.hip.  The clover term of the O(a)-improved Wilson operator (Sheikholeslami & Wohlert; Luescher,
 * Sint, Sommer & Weisz) and the kernels of its even-odd preconditioned solve:
 *   M_sw = A - kappa H,   A(x) = 1 + kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) Fhat_{mu nu}(x),
 * H the hop of l2q_su3_wilson_apply, sigma_{mu nu} = (i/2) [gamma_mu, gamma_nu] in its gamma basis, Fhat_{mu nu} =
 * (Q_{mu nu} - Q_{mu nu}^H) / 8 with Q_{mu nu} the sum of the four clover leaves of l2q_su3_clover_reduce (L1 = U_mu(x)
 * U_nu(x+mu) U_mu(x+nu)^H U_nu(x)^H).  Fhat is NOT made traceless: the definition for which published c_sw hold; M_sw is
 * 2 kappa times D_W + c_sw (i/4) sum_{mu,nu} sigma_{mu nu} Fhat_{mu nu}.  In the chiral basis A(x) = diag(A+, A-), two
 * Hermitian 6 x 6 blocks (row index 3 spin + colour within a chirality; A+ on spin 0, 1); with E_k = Fhat_{0k} and B =
 * (Fhat_23, -Fhat_13, Fhat_12):
 *   A+ = 1 - i kappa c_sw sum_k sigma_k (x) (E_k + B_k),   A- = 1 + i kappa c_sw sum_k sigma_k (x) (E_k - B_k).
 * A is Hermitian and commutes with gamma5, so M_sw^H = gamma5 M_sw gamma5 and the dagger bit of the hop still gives the
 * adjoint.  All four extents even (2 is legal), L2Q_ESHAPE otherwise.
 * Block field: cl[nb][2 parity][2 chirality][36][V/2] doubles, parity-ordered like x32 above: entry h of parity p is the
 * site of parity p of the pair (2h, 2h + 1).  The 36 reals of a block: its 6 diagonal entries, then (re, im) of the 15
 * entries above the diagonal, row-major.  The asymmetric even-odd form:
 *   Mhat = A_ee - kappa^2 H_eo A_oo^-1 H_oe,   bhat_e = b_e + kappa H_eo A_oo^-1 b_o,
 *   psi_o = A_oo^-1 (b_o + kappa H_oe psi_e);
 * with psi_o reconstructed, b - M_sw psi is bhat_e - Mhat psi_e on the even sites and 0 on the odd ones.
 * l2q_su3_clover_term: cl = A of both parities from the native links xn, coef = kappa c_sw (0 gives A = 1).  One thread
 * per site; once per configuration.  L2Q_EINVAL: a null pointer; cl aliasing xn; a non-positive size; coef not finite. */
int l2q_su3_clover_term(const void* xn, void* cl, double coef, int nb, int T, int X, int Y, int Z, void* stream);
/* clinv = the inverse of every block of cl, in the same layout, by an unpivoted L D L^H (no square roots).
 * minpiv_part[nb][2 parity][ceil((V/2) / 256)]: the smallest pivot d_i of a workgroup's blocks; logdet_part (may be null),
 * the same shape: its sum of log d_i (log det A of a parity = the sum of its partials), both by the fixed tree of the norm
 * partials.  A non-positive pivot is no error here: the minimum reports it, and the entries of that block are not
 * meaningful.  L2Q_EINVAL: a null cl, clinv or minpiv_part; outputs aliasing cl or each other; a non-positive size. */
int l2q_su3_clover_invert(const void* cl, void* clinv, double* minpiv_part, double* logdet_part, int nb, int T, int X,
                          int Y, int Z, void* stream);
/* l2q_su3_wilson_hop_eo with a block field c (A or its inverse; the blocks of `parity`, the parity of out, are read):
 *   cmode 0   out = b aux + a H src           c null: the hop itself
 *   cmode 1   out = b (C aux) + a H src
 *   cmode 2   out = C (b aux + a H src)
 * C(x) the block pair of c at the output site.  Everything else -- the arguments, flags, parity, aux and norm_part may be
 * null, out may be aux, the workgroup order with the right-hand side fastest -- as there.  Uses: the first half of Mhat
 * (cmode 2, c = A^-1, parity 1, no aux, a = 1); the second half (cmode 1, c = A, parity 0, a = -kappa^2, b = 1); the
 * reconstruction (cmode 2, c = A^-1, parity 1, a = kappa, b = 1); a parity of M_sw itself (cmode 1, c = A, a = -kappa,
 * b = 1).  Per (system, half-site) 504 flops for the two blocks on top of the hop's, and 576 B of blocks, which the nrhs
 * systems of a chain share.  L2Q_EINVAL as l2q_su3_wilson_hop_eo, and: cmode outside 0..2; c null with cmode 1 or 2, or
 * given with cmode 0; out aliasing c.  L2Q_ESHAPE: an odd extent. */
int l2q_su3_wilson_clover_hop_eo(const void* xn, const void* src, const void* aux, const void* c, void* out,
                                 double* norm_part, double a, double b, int flags, int parity, int cmode, int nb,
                                 int nrhs, int T, int X, int Y, int Z, void* stream);
/* out = C src on the half field [nb][nrhs][12][V/2] of `parity`, C the blocks of that parity of c; out may be src.
 * norm_part as above (may be null).  L2Q_EINVAL: a null c, src or out; out aliasing c; sizes and parity as above.
 * L2Q_ESHAPE: an odd extent. */
int l2q_su3_clover_apply(const void* c, const void* src, void* out, double* norm_part, int parity, int nb, int nrhs,
                         int T, int X, int Y, int Z, void* stream);
/* csrc/su3_clover_force.hip.  The clover part of the force of two flavours of dynamical clover quarks per pseudofermion
 * field, in the asymmetric even-odd form (Jansen & Liu), conventions of l2q_su3_wilson_force (dU/dt = p U, dS/dt = sum
 * <p, F>):
 *   S_f = sum_r phi_e,r^H (Mhat^H Mhat)^-1 phi_e,r - 2 npf log det A_oo,   det M_sw = det A_oo det Mhat.
 * With X_e = (Mhat^H Mhat)^-1 phi_e and Y_e = Mhat X_e completed by X_o = kappa A_oo^-1 H_oe X_e and
 * Y_o = kappa A_oo^-1 (H^H)_oe Y_e (one l2q_su3_wilson_clover_hop_eo each: cmode 2, c = A^-1, parity 1, the second with
 * the dagger bit),
 *   dS_pf  = -2 Re[Y^H dM_sw X] = 2 kappa Re[Y^H dH X] - 2 Re sum_x Y(x)^H dA(x) X(x),
 *   dS_det = -2 npf sum_{x odd} tr[A^-1(x) dA(x)],   dA(x) = kappa c_sw i sum_{mu<nu} sigma_{mu nu} (x) dFhat_{mu nu}(x).
 * The hop part is l2q_su3_wilson_force on the merged (X, Y).  This entry is the rest: with a b^H the colour outer product
 * summed over spin and
 *   Lambda_{mu nu}(x) = i sum_r (sigma_{mu nu} X_r)(x) Y_r(x)^H + [x odd] det_weight i tr_spin[sigma_{mu nu} A^-1(x)],
 * it is -2 kc sum_x sum_{mu<nu} Re tr[dFhat_{mu nu}(x) Lambda_{mu nu}(x)], kc = kappa c_sw.  Only the anti-Hermitian part of
 * Lambda contributes (with its trace: Fhat keeps its own), and Re tr(Lambda dFhat) = 1/4 Re tr(Lambda_AH dQ).
 *   f_out = (f_in ? f_in : 0) + coef F_sw,   F_sw = -TAH(U_mu(x) B_mu(x)),   dS = sum Re tr(B_mu(x) dU_mu(x)),
 * f_in, coef and the in-place use (f_in == f_out) as in l2q_su3_wilson_force; F_sw is stored exactly anti-Hermitian.
 * X, Y: full native fields [nb][npf][12][V], or both null with npf = 0: the determinant term alone.  clinv: the block
 * field of A^-1 (l2q_su3_clover_invert; its parity-1 half is read, entry s >> 1 for the odd site s), or null: the
 * pseudofermion term alone.  det_weight multiplies the determinant term: npf of the action above.
 * Two kernels, both gathers, no atomics: one thread per (chain, site) writes G = -(kc / 2) Lambda_AH as 6 planes x 9 reals
 * into ws[nb][6][9][V] (planes (01) (23) (02) (13) (03) (12); npf * 384 B of spinors and 2 x 288 B of blocks on odd sites
 * in, 432 B out), the sum over r in its order; one thread per link inserts G into the four clover leaves (the gather of
 * l2q_su3_clover_bwd) and projects.  A chain's force is the same bits alone and in a batch, and from run to run.  All
 * four extents even (2 is legal: every geometric occurrence is its own term, as in the forward), L2Q_ESHAPE otherwise.
 * ws_bytes >= nb * 54 * V * sizeof(double).
 * L2Q_EINVAL, before any HIP call: a null xn, f_out or ws; X or Y null with npf > 0 or given with npf = 0, npf < 0; both
 * halves absent (npf = 0 and clinv null); f_out aliasing xn, X, Y, clinv or ws; ws aliasing xn, X, Y, clinv or f_in; a
 * non-positive size; nb * npf * 12 * V of 2^31 or more; kc, coef or det_weight not finite; the workspace too small. */
int l2q_su3_clover_force(const void* xn, const void* X, const void* Y, const void* clinv, const void* f_in, void* f_out,
                         double kc, double coef, double det_weight, int nb, int npf, int T, int X_, int Y_, int Z,
                         void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- L2HMC momentum update */
/* Generalised v-update with real network heads s, t, q [nb][n] applied entry-wise:
 *   forward : v' = exp(eps s/2) v - (eps/2) (F exp(eps q) + t),  logdet[c] =  sum eps s/2
 *   backward: v' = exp(-eps s/2) (v + (eps/2) (F exp(eps q) + t)), logdet[c] = -sum eps s/2
 * (dynamics.py:1266-1297).  is_complex=1: v, F are complex128 [nb][n] (SU3, heads multiply
 * both parts, t adds to the real part); 0: real.  elem_bytes 8 (f64) or 4 (f32, U1).
 * v is updated in place. */
int l2q_v_update(void* v, const void* force, const void* s, const void* t, const void* q,
                 double eps, int forward, int is_complex, int elem_bytes, int nb, long n,
                 void* logdet, void* ws, size_t ws_bytes, void* stream);
/* The same update out of place: v_out = update(v_in) (v_in is not written; v_out == v_in is the
 * in-place call).  The training tape keeps the momentum BEFORE every update for its reverse sweep:
 * this saves the copy. */
int l2q_v_update_to(const void* v_in, void* v_out, const void* force, const void* s, const void* t,
                    const void* q, double eps, int forward, int is_complex, int elem_bytes, int nb,
                    long n, void* logdet, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- accept / reject */
/* acc = exp(min(0, h_init - h_prop + sumlogdet)); mask = (acc > u) as float32 0/1
 * (dynamics.py:1065-1087).  elem_bytes of h/sumlogdet/acc/u: 8 or 4. */
int l2q_accept(const void* h_init, const void* h_prop, const void* sumlogdet, const void* u,
               void* acc, float* mask, int nb, int elem_bytes, void* stream);
/* out[c][:] = mask[c] ? a[c][:] : b[c][:]   (dynamics.py:677-682), row_bytes (multiple of 4)
 * per chain */
int l2q_select_rows(const void* a, const void* b, const float* mask, void* out, int nb,
                    long row_bytes, void* stream);
/* y = alpha * x over n doubles (momentum flip, dynamics.py:1001); y may alias x */
int l2q_scale_f64(const double* x, double alpha, double* y, long n, void* stream);

/* ---------------------------------------------------------------- dense network layers */
/* C[M][N] = epilogue( A[M][K] . W[N][K]^T (+ A2[M][K2] . W2[N][K2]^T) + bias[N] (+ bias2[N]) )
 * fp64 on v_mfma_f64_16x16x4_f64.  Replaces nn.Linear + activation / ScaledTanh in
 * LeapfrogLayer.forward (network/pytorch/network.py:430-451, 522-551):
 *   epilogue: y = act(z);  if (coeff) y = scale * exp(coeff[n]) * y  else y = scale * y.
 * A2/W2/bias2 may be NULL (K2 = 0).  ws: split-K scratch (l2q_gemm_ws_bytes). */
int l2q_gemm_f64(const double* A, const double* W, int M, int N, long K, const double* A2,
                 const double* W2, long K2, const double* bias, const double* bias2,
                 const double* coeff, double scale, int act, double* C, void* ws,
                 size_t ws_bytes, void* stream);
size_t l2q_gemm_ws_bytes(int M, int N, long K, long K2);
/* The same layer (fp64 operands and result) with the products rebuilt from exact int8 x int8 -> int32 digit
 * products on v_mfma_i32_16x16x64_i8 (csrc/gemm_sliced.hip) -- for the input layer of the
 * SU(3) vnet, whose K = 64 V runs to 2 x 131 072 at 8^4 (network/pytorch/network.py:430-451, xlayer + vlayer).
 * l2q_gemm_sliced_build turns one weight matrix W [N][K] into its digit image (l2q_gemm_sliced_bytes(N, K)
 * bytes, 256-byte aligned: 7 int8 planes in MFMA fragment order + one power-of-two scale per output row;
 * rebuild when W changes; *usable = 0 for a non-finite entry; the call synchronises the stream).
 * l2q_gemm_sliced_f64 slices the activations ON THE FLY against ONE exponent per operand: every entry of A must
 * satisfy |a| < 2^a_exp (A2: a2_exp) -- the vnet inputs su3_to_vec(projectSU(.)) do with a_exp = 2 --; a value
 * outside the range or a NaN turns the whole output into NaN (as a NaN operand would).  Needs M, N multiples of
 * 64 and K, K2 multiples of 64.  Results agree with l2q_gemm_f64 to the accumulation error of that kernel
 * (not bit for bit).  A2 / image2 may be NULL (K2 = 0). */
size_t l2q_gemm_sliced_bytes(int N, long K);
int l2q_gemm_sliced_build(const double* W, int N, long K, void* image, size_t image_bytes, int* usable,
                          void* stream);
size_t l2q_gemm_sliced_ws_bytes(int M, int N, long K, long K2);
int l2q_gemm_sliced_f64(const double* A, const void* image, long K, int a_exp, const double* A2,
                        const void* image2, long K2, int a2_exp, int M, int N, const double* bias,
                        const double* bias2, const double* coeff, double scale, int act, double* C, void* ws,
                        size_t ws_bytes, void* stream);
/* l2q_gemm_sliced_f64 with the activations given as digit images too (csrc/gemm_digits.hip, csrc/digits.hpp:
 * [M][K / 64][7][64] bytes, l2q_gemm_digits_bytes(M, K) of them, 16-byte aligned), written by
 * l2q_gemm_digits_slice from fp64 A [M][K] or by the kernels that produce the activations
 * (l2q_su3_projsu_digits, l2q_su3_expm_mul2_digits): the digits are made once instead of once per column tile.
 * Same digits, sums and reduce as l2q_gemm_sliced_f64: the same bits.  A value outside (-2^a_exp, 2^a_exp) or a
 * NaN seen by a producer turns the output of the next sliced layer launched on the device into NaN.  Workspace:
 * l2q_gemm_sliced_ws_bytes. */
size_t l2q_gemm_digits_bytes(long M, long K);
int l2q_gemm_digits_slice(const double* A, long M, long K, int a_exp, void* image, size_t image_bytes, void* stream);
int l2q_gemm_digits_f64(const void* A, const void* image, long K, int a_exp, const void* A2, const void* image2,
                        long K2, int a2_exp, int M, int N, const double* bias, const double* bias2,
                        const double* coeff, double scale, int act, double* C, void* ws, size_t ws_bytes,
                        void* stream);
/* The three output heads of a LeapfrogLayer AND the generalised momentum update in one kernel
 * (network.py:547-551 + dynamics.py:1266-1297): for chain m, entry n
 *   s = cs[n] tanh(Z.Ws[n] + bs[n]);  t = scale_t (Z.Wt[n] + bt[n]);  q = cq[n] tanh(Z.Wq[n] + bq[n])
 *   v' and logdet as in l2q_v_update.   s, t, q are never written to memory.
 * cs / cq: per-entry scale nw.s * exp(coeff_s[n]) (NULL -> the scalar scale_s / scale_q).
 * Z [M][K] (K even), W* [N][K], v / force [M][N] real or complex128, logdet [M]. */
int l2q_vnet_heads_vupdate_f64(const double* Z, int M, int K, long N, const double* Ws,
                               const double* bs, const double* cs, double scale_s,
                               const double* Wt, const double* bt, double scale_t,
                               const double* Wq, const double* bq, const double* cq,
                               double scale_q, void* v, const void* force, int is_complex,
                               double eps, int forward, double* logdet, void* ws,
                               size_t ws_bytes, void* stream);
/* The same update out of place: the momentum is read from v_in and written to v_out (v_in == v_out
 * is the in-place call; any other overlap is undefined).  A trajectory's first update uses it to
 * leave the momentum it was handed untouched without copying it. */
int l2q_vnet_heads_vupdate_to_f64(const double* Z, int M, int K, long N, const double* Ws,
                                  const double* bs, const double* cs, double scale_s,
                                  const double* Wt, const double* bt, double scale_t,
                                  const double* Wq, const double* bq, const double* cq,
                                  double scale_q, const void* v_in, void* v_out, const void* force,
                                  int is_complex, double eps, int forward, double* logdet, void* ws,
                                  size_t ws_bytes, void* stream);
/* Two consecutive v-updates on the SAME x (closing update of leapfrog step k, opening update
 * of step k+1; optionally the merged trajectory's momentum flip v -> -v in between,
 * dynamics.py:1001) from ONE evaluation of the heads: update (eps1, forward1), [flip],
 * update (eps2, forward2).  logdet receives the sum of both updates' log-Jacobians. */
int l2q_vnet_heads_vupdate_pair_f64(const double* Z, int M, int K, long N, const double* Ws,
                                    const double* bs, const double* cs, double scale_s,
                                    const double* Wt, const double* bt, double scale_t,
                                    const double* Wq, const double* bq, const double* cq,
                                    double scale_q, void* v, const void* force, int is_complex,
                                    double eps1, int forward1, int flip_between, double eps2,
                                    int forward2, double* logdet, void* ws, size_t ws_bytes,
                                    void* stream);
/* The same pair of updates with what per-step metrics need of the state BETWEEN them
 * (dynamics.py:865-886 evaluates the Hamiltonian after every leapfrog step): logdet1 [M] = the first
 * update's log-Jacobian alone (logdet still receives the sum), vnorm2_mid [M] = sum |v|^2 of the
 * momentum after the first update (before the flip, which does not change it).  Needs K % 16 == 0. */
int l2q_vnet_heads_vupdate_pair_mid_f64(const double* Z, int M, int K, long N, const double* Ws,
                                        const double* bs, const double* cs, double scale_s,
                                        const double* Wt, const double* bt, double scale_t,
                                        const double* Wq, const double* bq, const double* cq,
                                        double scale_q, void* v, const void* force, int is_complex,
                                        double eps1, int forward1, int flip_between, double eps2,
                                        int forward2, double* logdet, double* logdet1,
                                        double* vnorm2_mid, void* ws, size_t ws_bytes, void* stream);
size_t l2q_vnet_heads_ws_bytes(int M, long N);
/* The same heads + momentum update with the fp64 products rebuilt from exact int8 x int8 -> int32 slice
 * products on v_mfma_i32_16x16x64_i8 (error-free slicing, csrc/heads_sliced.hip): an
 * inference path for K = 256 (the reference's default width of the last hidden layer of the SU(3) nets).
 * l2q_heads_sliced_build turns the three weight matrices [N][K] into the int8 slice image + per-entry
 * power-of-two scales (sliced: l2q_heads_sliced_bytes(K, N) bytes, 256-byte aligned; rebuild when the
 * weights change); *usable = 0 when a weight vector's dynamic range is too wide for the 54-bit fixed
 * point (mean |w| below 2^-6 of the largest): keep the fp64 kernel then.  The call synchronises the
 * stream.  l2q_vnet_heads_vupdate_sliced_f64 is the four fp64 entry points in one: v_in NULL = in
 * place; pair = 0 ignores flip_between / eps2 / forward2; logdet1 / vnorm2_mid non-NULL (pair only) =
 * the mid-point outputs; pair = 0 with logdet1 NULL and vnorm2_mid non-NULL: vnorm2_mid [M] = sum |v_out|^2 of
 * the momentum the single update writes (v and logdet are the same bits with or without the request).
 * Results agree with the fp64 kernels to fp64 rounding (not bit for bit).
 * The per-call operand Z gets the same conditioning test as the weights, as a DIAGNOSTIC: rows whose
 * mean |z| is below 2^-6 of their largest entry (possible with an unbounded activation; never with
 * tanh) are counted per device -- their products are exact to 2^-54 K max|z| max|w| rather than to
 * fp64 rounding of sum |z||w|.  l2q_heads_sliced_zflag copies the count to *count (host), optionally
 * resets it, and synchronises the stream. */
size_t l2q_heads_sliced_bytes(int K, long N);
int l2q_heads_sliced_zflag(int reset, int* count, void* stream);
int l2q_heads_sliced_build(const double* Ws, const double* Wt, const double* Wq, int K, long N, void* sliced,
                           size_t sliced_bytes, int* usable, void* stream);
size_t l2q_vnet_heads_sliced_ws_bytes(int M, long N);
int l2q_vnet_heads_vupdate_sliced_f64(const double* Z, int M, int K, long N, const void* sliced,
                                      const double* bs, const double* cs, double scale_s, const double* bt,
                                      double scale_t, const double* bq, const double* cq, double scale_q,
                                      const void* v_in, void* v, const void* force, int is_complex, double eps1,
                                      int forward1, int pair, int flip_between, double eps2, int forward2,
                                      double* logdet, double* logdet1, double* vnorm2_mid, void* ws,
                                      size_t ws_bytes, void* stream);
/* The same call with one more property of `force`.  force_upper = 1: force is an upper-plane SU(3) force
 * [M][4][6][V] (l2q_su3_force_upper) instead of the full [M][N] field; needs is_complex, N = 36 V, V % 64 == 0 and
 * M * 192 * V < 2^32.  The kernel reads the three planes that are not stored from their transposes' planes and
 * flips the sign of the real part: the results are those of the full field bit for bit, except that a real part
 * that is an exact zero off the diagonal enters as the other zero (visible only where the t head is an exact zero
 * as well).  force_upper = 0: l2q_vnet_heads_vupdate_sliced_f64 itself (V is not read). */
int l2q_vnet_heads_vupdate_sliced_upper_f64(const double* Z, int M, int K, long N, const void* sliced,
                                            const double* bs, const double* cs, double scale_s, const double* bt,
                                            double scale_t, const double* bq, const double* cq, double scale_q,
                                            const void* v_in, void* v, const void* force, int is_complex,
                                            double eps1, int forward1, int pair, int flip_between, double eps2,
                                            int forward2, double* logdet, double* logdet1, double* vnorm2_mid,
                                            void* ws, size_t ws_bytes, int force_upper, long V, void* stream);
/* The forward pass of the TRAINING tape on the same kernel (network.py:547-551 + dynamics.py:1266-1297 under
 * autograd: trainers/pytorch/trainer.py:1316-1367): one (not paired) out-of-place v-update v_in -> v AND the
 * three heads as the update uses them -- s = cs tanh(.), t = scale_t (.), q = cq tanh(.), [M][N] fp64 each --
 * for the reverse sweep (l2q_v_update_bwd_c128, the heads' VJPs).  The slice image is rebuilt once per
 * optimiser step from that step's weights (l2q_heads_sliced_build).  Same workspace as the call above. */
int l2q_vnet_heads_vupdate_sliced_tape_f64(const double* Z, int M, int K, long N, const void* sliced,
                                           const double* bs, const double* cs, const double* bt, double scale_t,
                                           const double* bq, const double* cq, const void* v_in, void* v,
                                           const void* force, int is_complex, double eps, int forward,
                                           double* s_out, double* t_out, double* q_out, double* logdet, void* ws,
                                           size_t ws_bytes, void* stream);
/* fp32 variant on v_mfma_f32_16x16x4_f32 (U(1) networks). */
int l2q_gemm_f32(const float* A, const float* W, int M, int N, long K, const float* A2,
                 const float* W2, long K2, const float* bias, const float* bias2,
                 const float* coeff, float scale, int act, float* C, void* ws,
                 size_t ws_bytes, void* stream);
/* Backward GEMMs of the dense layers without transposed copies (the reverse sweep of the training
 * step):  C[M][N] (+)= sum_k Aop[m][k] Wop[n][k]  with  Aop[m][k] = a_trans ?
 * A[k][m] (A stored [K][M]) : A[m][k] (A stored [M][K]), Wop likewise ([K][N] resp. [N][K]).
 *   dW += dY^T X : A = dY [nb][out] (a_trans), W = X [nb][in] (w_trans), accumulate
 *   dX  = dY W   : A = dY [nb][out],           W = W [out][in] (w_trans)
 * elem_bytes 4 | 8.  Transposed operands need their row length (M resp. N) to be a multiple of
 * 16 bytes.  ws: l2q_gemm_ws_bytes(M, N, K, 0). */
int l2q_gemm_ex(const void* A, int a_trans, const void* W, int w_trans, int M, int N, long K,
                int elem_bytes, int accumulate, void* C, void* ws, size_t ws_bytes, void* stream);
/* Half-precision network layers ("fp16 nets / fp32 action", BASELINE cfg-3): what the reference
 * gets from torch.autocast around Dynamics.forward (trainers/pytorch/trainer.py:211-219,
 * 1278-1280: nn.Linear in fp16 / bf16, lattice arithmetic in fp32).  W / W2 are 16-bit
 * (half_type: L2Q_HALF_F16 | L2Q_HALF_BF16), A / A2 16-bit or fp32 (a_is_f32: rounded to 16 bit
 * as the tile is staged, no cast pass), C 16-bit or fp32 (c_is_f32); bias / bias2 / coeff fp32.
 * fp32 accumulation on v_mfma_f32_16x16x32_{f16,bf16}.  Rounding points as autocast has them:
 *   y = r16(acc + bias);  y = r16(act(y));  C = coeff ? scale * exp(coeff[n]) * y : r16(scale * y)
 * (coeff needs c_is_f32: torch promotes fp32 x fp16 tensors to fp32).  ws: split-K scratch of
 * l2q_gemm_h_ws_bytes. */
int l2q_gemm_h(int half_type, const void* A, int a_is_f32, const void* W, int M, int N, long K,
               const void* A2, const void* W2, long K2, const float* bias, const float* bias2,
               const float* coeff, float scale, int act, void* C, int c_is_f32, void* ws,
               size_t ws_bytes, void* stream);
size_t l2q_gemm_h_ws_bytes(int M, int N, long K, long K2);
/* K-splits the streaming input-layer kernel (fp32 A / A2, N <= 256, wide K: csrc/gemm_f16_skinny.hip) takes for
 * this shape under the current `gemm_h_skinny` tuning; 0: the tile kernels run it.  K as passed to l2q_gemm_h
 * (u1x: 2 xdim). */
int l2q_gemm_h_skinny_splits(int M, int N, long K, long K2, int u1x);
/* The U(1) xnet's input layer in half precision with its [cos(m x), sin(m x)] input
 * (dynamics.py:1161-1185, network.py:430-451) formed inside the GEMM's tile loader:
 *   C = r16(act(r16([cos(keep x) | sin(keep x)] . W^T + A2 . W2^T + bias + bias2))),
 * x [M][xdim] fp32 link angles, keep = mask[xdim] (complement: 1 - mask), W [N][2 xdim] 16-bit,
 * A2 [M][K2] fp32 (the momenta), W2 [N][K2] 16-bit, C [M][N] 16-bit.
 * ws: l2q_gemm_h_ws_bytes(M, N, 2 xdim, K2). */
int l2q_gemm_h_u1x(int half_type, const float* x, const float* mask, int complement, const void* W,
                   int M, int N, long xdim, const float* A2, const void* W2, long K2,
                   const float* bias, const float* bias2, int act, void* C, void* ws,
                   size_t ws_bytes, void* stream);
/* The three heads of a half-precision U(1) LeapfrogLayer and the sub-update that consumes them
 * in one kernel (network.py:547-551 + dynamics.py:1266-1297 / 1386-1477); s, t, q never reach
 * memory.  Z [M][K] 16-bit (last hidden activation), W* [N][K] 16-bit, b* fp32 [N],
 * cs / cq = nw * exp(coeff) fp32 [N] (rounding points as l2q_gemm_h):
 *   x_update == 0: a = v (in place), b = force:  l2q_v_update's arithmetic
 *   x_update != 0: a = x (in place), b = v, mask [N] / complement:  l2q_u1_x_update's
 * logdet [M] fp32 (accumulate != 0: added to).  ws: l2q_u1_heads_update_h_ws_bytes. */
int l2q_u1_heads_update_h(int half_type, const void* Z, int M, int K, long N, const void* Ws,
                          const float* bs, const float* cs, const void* Wt, const float* bt,
                          float scale_t, const void* Wq, const float* bq, const float* cq,
                          int x_update, float* a, const float* b, const float* mask,
                          int complement, float eps, int forward, int use_ncp, float* logdet,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);
size_t l2q_u1_heads_update_h_ws_bytes(int M, long N);
/* Half-precision ConvStack layers (autocast runs nn.Conv2d in 16 bit too, network.py:283-326):
 * l2q_conv_gemm_periodic_f32's implicit GEMM on the 16-bit MFMA.  in: fp32 (in_is_f32, the first
 * layer's [cos, sin] lattice data, rounded while staged) or 16-bit; weight [cout][C k k] 16-bit in
 * (ci, i, j) or, channels_last_cols != 0, (i, j, ci) order; bias fp32; out NHWC 16-bit
 * = r16(act(r16(conv + bias))).  l2q_maxpool_act_nhwc_h: MaxPool2d(pool) then activation on NHWC
 * 16-bit data. */
int l2q_conv_gemm_periodic_h(int half_type, const void* in, int in_is_f32, long sn, long sc, long sh,
                             long sw, int nb, int C, int H, int W, int k, const void* weight,
                             int channels_last_cols, const float* bias, int cout, int act,
                             void* out, void* stream);
/* l2q_conv_gemm_periodic_h followed by MaxPool2d(2) (floor mode) and the activation, in one kernel
 * (network.py:283-326: Conv2d -> MaxPool2d -> act of the pooled ConvStack layers): out is the pooled
 * NHWC image [nb][Ho / 2][Wo / 2][cout] = r16(act(max_window r16(conv + bias))); the un-pooled image
 * is never written.  Same bits as l2q_conv_gemm_periodic_h (act none) + l2q_maxpool_act_nhwc_h(2). */
int l2q_conv_pool_gemm_periodic_h(int half_type, const void* in, int in_is_f32, long sn, long sc,
                                  long sh, long sw, int nb, int C, int H, int W, int k,
                                  const void* weight, int channels_last_cols, const float* bias,
                                  int cout, int act, void* out, void* stream);
int l2q_maxpool_act_nhwc_h(int half_type, const void* in, int nb, int H, int W, int C, int pool,
                           int act, void* out, void* stream);
/* out[b][h][w][c] = c < C ? r16(in[b][c][h][w]) : 0 for c < cpad: the fp32 NCHW lattice input of
 * the first conv layer as 16-bit NHWC with the channels padded to a 16-byte group. */
int l2q_nchw_to_nhwc_pad_h(int half_type, const float* in, int nb, int C, int H, int W, int cpad,
                           void* out, void* stream);

/* ---------------------------------------------------------------- U(1) lattice kernels */
/* x[nb][2][T][X] angles, elem_bytes 4 or 8.
 * out[c][0] = sum cos(theta), [1] = sum sin(theta), [2] = sum project_angle(theta)
 * (lattice/u1/pytorch/lattice.py:154-159, 80-86, 188-228):
 *   action = beta (V - out0); plaqs = out0/V; sinQ = out1/2pi; intQ = out2/2pi. */
int l2q_u1_plaq_reduce(const void* x, int nb, int T, int X, int elem_bytes, void* out,
                       void* stream);
/* The plaquette-angle field out[c][t][x] = U0(t,x) + U1(t+1,x) - U0(t,x+1) - U1(t,x): the tensor [nb, T, X]
 * that LatticeU1.wilson_loops returns (lattice/u1/pytorch/lattice.py:154-159). */
int l2q_u1_wilson_loops(const void* x, int nb, int T, int X, int elem_bytes, void* out, void* stream);
/* its adjoint (VJP): dx0(t,x) += g(t,x) - g(t,x-1), dx1(t,x) += g(t-1,x) - g(t,x);  g [nb][T][X] */
int l2q_u1_wilson_loops_bwd(const void* g, int nb, int T, int X, int elem_bytes, void* dx, void* stream);
/* F0 = beta [sin th - sin th(t,x-1)], F1 = beta [-sin th + sin th(t-1,x)]
 * (autograd of the action, lattice.py:102-117).  If v != NULL: v += coef * F (fused kick)
 * and `force` may be NULL. */
int l2q_u1_force(const void* x, double beta, void* force, void* v, double coef, int nb, int T,
                 int X, int elem_bytes, void* stream);
/* NCP position update (dynamics.py:1386-1477, use_ncp branch) followed by compat_proj:
 *   forward : x' = m x + (1-m) [2 atan(tan(x/2) e^{eps s}) + eps (v e^{eps q} + t)]
 *   backward: x' = m x + (1-m) [2 atan(tan(x/2) e^{-eps s}) - e^{-eps s} eps (v e^{eps q} + t)]
 *   logdet[c] = sum (1-m) log(e^{+-eps s} / (cos^2(x/2) + e^{+-2 eps s} sin^2(x/2)))
 * mask: float32 [n] (the kept entries; complement flips it).  x updated in place. */
int l2q_u1_x_update(void* x, const void* v, const void* s, const void* t, const void* q,
                    const float* mask, int complement, double eps, int forward, int use_ncp,
                    int elem_bytes, int nb, long n, void* logdet, void* stream);
/* ((x + pi) mod 2 pi) - pi   (group/u1/pytorch/group.py:137-138); y may alias x */
int l2q_u1_wrap(const void* x, void* y, long n, int elem_bytes, void* stream);
/* out[c] = 0.5 sum v^2 (group/u1/pytorch/group.py:164-165) */
int l2q_u1_kinetic_reduce(const void* v, int nb, long n, int elem_bytes, void* out,
                          void* stream);
/* y = x + alpha * p  (U1Phase.update_gauge, group.py:102-103) */
int l2q_axpy(const void* p, double alpha, void* x, long n, int elem_bytes, void* stream);
/* [cos(m x), sin(m x)] channels for the U(1) xnet input (group.py:86-89 applied to the
 * masked field, dynamics.py:1398,1174): out[nb][4][T*X] from x[nb][2][T*X] */
int l2q_u1_masked_cos_sin(const void* x, const float* mask, int complement, void* out, int nb,
                          long n, int elem_bytes, void* stream);
/* periodic-padded conv2d (+ optional max-pool p, + activation), NCHW fp32:
 * PeriodicPadding(k-1) -> Conv2d(k) -> [MaxPool2d(p)] -> [act]
 * (network/pytorch/network.py:151-172, 283-326). */
int l2q_conv2d_periodic_f32(const float* in, const float* w, const float* bias, float* out,
                            int nb, int cin, int H, int W, int cout, int k, int pool, int act,
                            void* stream);

/* The same conv layer as an implicit GEMM (the fast path of ConvStack): periodic im2col
 *   col[(b*Ho + ho)*Wo + wo][(ci*k + i)*k + j] = in[b, ci, (ho+i-k+1) mod H, (wo+j-k+1) mod W]
 * with Ho = H+k-1, Wo = W+k-1 and generic element strides (sn, sc, sh, sw) of `in` (NCHW for
 * the first layer, the GEMM's NHWC output afterwards); then l2q_gemm_f32(col, weight[cout][cin k k])
 * gives the NHWC activation; l2q_maxpool_act_nhwc_f32 applies MaxPool2d(pool) + activation.
 * channels_last_cols != 0: column order (i*k + j)*C + ci instead (weight permuted to
 * [cout][k][k][C]): contiguous runs over the channels of an NHWC input, for im2col and for its
 * adjoint l2q_col2im_periodic_f32 alike. */
int l2q_im2col_periodic_f32(const float* in, long sn, long sc, long sh, long sw, int nb, int C,
                            int H, int W, int k, int channels_last_cols, float* col,
                            void* stream);
int l2q_maxpool_act_nhwc_f32(const float* in, int nb, int H, int W, int C, int pool, int act,
                             float* out, void* stream);
/* fp64 twins (the conv stack under precision=float64) */
int l2q_im2col_periodic_f64(const double* in, long sn, long sc, long sh, long sw, int nb, int C,
                            int H, int W, int k, int channels_last_cols, double* col,
                            void* stream);
int l2q_maxpool_act_nhwc_f64(const double* in, int nb, int H, int W, int C, int pool, int act,
                             double* out, void* stream);
/* The conv layer without the col matrix: im2col happens inside the A-tile loader of the f32
 * MFMA GEMM.  out[(b*Ho + ho)*Wo + wo][cout] = act(conv + bias) (NHWC); weight [cout][C k k] in
 * nn.Conv2d's flatten order (ci, i, j), or -- channels_last_cols != 0 -- permuted to (i, j, ci) so
 * that consecutive K columns of an NHWC input are contiguous in memory; input strides as for
 * l2q_im2col_periodic_f32.  (The eval path uses
 * this; the training path keeps the materialised col matrix because the weight gradient needs it.) */
int l2q_conv_gemm_periodic_f32(const float* in, long sn, long sc, long sh, long sw, int nb, int C,
                               int H, int W, int k, const float* weight, int channels_last_cols,
                               const float* bias, int cout, int act, float* out, void* stream);
/* fp64: the same implicit GEMM on v_mfma_f64_16x16x4_f64 (16-byte gathers of two channels) */
int l2q_conv_gemm_periodic_f64(const double* in, long sn, long sc, long sh, long sw, int nb, int C,
                               int H, int W, int k, const double* weight, int channels_last_cols,
                               const double* bias, int cout, int act, double* out, void* stream);
/* out[b][h][w][c] = c < C ? in[b][c][h][w] : 0 for c < cpad (fp32 NCHW -> NHWC, channels padded
 * to a 16-byte group): lets the first conv layer use the vector gathers of the later ones. */
int l2q_nchw_to_nhwc_pad_f32(const float* in, int nb, int C, int H, int W, int cpad, float* out,
                             void* stream);
int l2q_nchw_to_nhwc_pad_f64(const double* in, int nb, int C, int H, int W, int cpad, double* out,
                             void* stream);

/* ---------------------------------------------------------------- fused U(1) sub-updates (fp32)
 * One launch per L2HMC sub-update on small 2D lattices (n = 2 T X <= l2q_u1_fused_max_n()):
 * the force (v-step) or the masked cos/sin inputs (x-step), the whole dense LeapfrogLayer in
 * eval mode (network.py:430-451, 522-551; BatchNorm folded into the heads by the caller) and
 * the update with its log-det (dynamics.py:1266-1297 / 1386-1477).  s, t, q never reach memory.
 * Network description (device pointers unless noted):
 *   wxT [Kx][U0], wvT [Kv][U0]   transposed xlayer / vlayer weights, b0 [U0] = sum of their biases
 *   hidden                       for l = 1..nl-1: W_l [U_l][U_{l-1}] then b_l [U_l], packed
 *   units (HOST pointer) [nl]    widths U_0..U_{nl-1} (each <= 64, nl <= 8)
 *   ws, wt, wq [n][U_last], bs, bt, bq [n]; cs, cq [n] per-entry scale (nw * exp(coeff));
 *   scale_t; act: L2Q_ACT_* of the dense layers.
 * v-step: Kx = Kv = n (inputs x and force(x)); v updated in place, x untouched.
 * x-step: Kx = 2 n ([cos(m x), sin(m x)]), Kv = n (v); x updated in place (+ compat_proj).
 * accumulate != 0: logdet[c] += the sub-update's log-det (running sum of a leapfrog step). */
int l2q_u1_fused_max_n(void);
int l2q_u1_vstep_f32(const float* x, float* v, double beta, double eps, int forward, int nb, int T,
                     int X, const float* wxT, const float* wvT, const float* b0,
                     const float* hidden, const int* units, int nl, const float* ws,
                     const float* bs, const float* cs, const float* wt, const float* bt,
                     double scale_t, const float* wq, const float* bq, const float* cq, int act,
                     int accumulate, float* logdet, void* stream);
int l2q_u1_xstep_f32(float* x, const float* v, const float* mask, int complement, double eps,
                     int forward, int use_ncp, int nb, int n, const float* wxT, const float* wvT,
                     const float* b0, const float* hidden, const int* units, int nl,
                     const float* ws, const float* bs, const float* cs, const float* wt,
                     const float* bt, double scale_t, const float* wq, const float* bq,
                     const float* cq, int act, int accumulate, float* logdet, void* stream);

/* ================================================================ training-gradient path
 * Reverse-mode (VJP) counterparts of the U(1) sub-updates and network layers, the train-mode
 * BatchNorm1d, and the optimiser step.  The reference gets these from torch.autograd
 * (`loss.backward()`, trainers/pytorch/trainer.py:1284-1314) and torch.optim.Adam (:206-209).
 * Conventions: "g*" / "d*" arguments are cotangents with the shape of the quantity they
 * belong to; arguments documented "+=" are accumulated into, all others are overwritten. */

/* y = act(x) element-wise (ACTIVATION_FNS, network.py:40-46); y may alias x.  The training tape
 * uses it for swish, whose derivative needs the pre-activation (the GEMM epilogues fuse the
 * activation and keep only its output). */
int l2q_act_fwd(const void* x, int act, long n, int elem_bytes, void* y, void* stream);
/* dx = dy * act'(z) from the activation OUTPUT y = act(z) (tanh, relu, leaky_relu, elu, none);
 * for swish (not invertible) `y` must hold the PRE-activation z.  dx may alias dy.
 * (network.py:447-451, 536-538) */
int l2q_act_bwd(const void* dy, const void* y, int act, long n, int elem_bytes, void* dx,
                void* stream);
/* l2q_act_bwd over y[M][N] with the bias gradient formed in the same pass: dz = dy * act'(y) (swish:
 * `y` holds the PRE-activation, as in l2q_act_bwd) and bgrad[n] += sum_m dz[m][n].  The column sums go
 * through double-precision partials over the row blocks of l2q_colsum, in a fixed order: the result
 * depends on (M, N) only, not on the launch grid.  dz holds the bits l2q_act_bwd gives and may alias
 * dy.  elem_bytes 4 | 8; ws_bytes >= l2q_colsum_ws_bytes(M, N).  The training tape uses it for the
 * un-pooled swish conv layers (M = chains x Ho x Wo rows of `cout` channels), where it replaces a copy
 * of dy, l2q_act_bwd and l2q_colsum. */
int l2q_act_bwd_sums(const void* dy, const void* y, int act, long M, int N, int elem_bytes, void* dz,
                     void* bgrad, void* ws, size_t ws_bytes, void* stream);
/* y = r16(act(r16(x))) element-wise on fp32 containers, r16 = round to half_type (L2Q_HALF_F16 |
 * L2Q_HALF_BF16) and back: torch.autocast's two rounding points around an activation, with the
 * conversion and the arithmetic of the l2q_gemm_h epilogues, so that a layer whose activation runs
 * here rounds like one whose activation is fused.  The 16-bit training tape uses it for swish: the
 * GEMM runs without its activation, the (16-bit valued) pre-activation stays on the tape.  y may
 * alias x. */
int l2q_act_fwd_r16(int half_type, const float* x, int act, long n, float* y, void* stream);
/* out = alpha * a * b element-wise (nn.Dropout mask, network.py:540-541); out may alias a */
int l2q_mul(const void* a, const void* b, double alpha, long n, int elem_bytes, void* out,
            void* stream);
/* y[c][:] += a[c] * x[c][:]  (cotangent of the kinetic energy 1/2 sum v^2, dynamics.py:1485) */
int l2q_axpy_rows(const void* x, const void* a, int nb, long n, int elem_bytes, void* y,
                  void* stream);
/* out[n] (+)= alpha * sum_m a[m][n] * (b ? b[m][n] : 1), fixed summation order
 * (bias gradients; ScaledTanh.coeff gradient with b = the head's output) */
int l2q_colsum(const void* a, const void* b, long M, int N, double alpha, int accumulate,
               int elem_bytes, void* out, void* ws, size_t ws_bytes, void* stream);
size_t l2q_colsum_ws_bytes(long M, int N);
/* head s = scale * exp(coeff[n]) * tanh(pre) (ScaledTanh, network.py:175-206):
 * dpre = ds * scale e^coeff (1 - tanh^2), tanh recovered from s.  coeff == NULL: linear head
 * t = scale * pre, dpre = scale * ds. */
int l2q_scaled_tanh_bwd(const void* ds, const void* s, const void* coeff, double scale, int M,
                        int N, int elem_bytes, void* dpre, void* stream);
/* l2q_scaled_tanh_bwd with the column sums of the head's parameter gradients formed in the same pass:
 * bgrad[n] += sum_m dpre[m][n] (nn.Linear bias) and, with coeff, cgrad[n] += sum_m ds[m][n] s[m][n]
 * (ScaledTanh.coeff) -- the bits of l2q_scaled_tanh_bwd + two l2q_colsum passes (same row partition and
 * summation order).  ws_bytes >= 2 * l2q_colsum_ws_bytes(M, N). */
int l2q_scaled_tanh_bwd_sums(const void* ds, const void* s, const void* coeff, double scale, int M, int N,
                             int elem_bytes, void* dpre, void* bgrad, void* cgrad, void* ws, size_t ws_bytes,
                             void* stream);
/* nn.BatchNorm1d in train mode over x[M][N] (network.py:543-544): batch mean / biased
 * variance, y = (x - mean) invstd gamma + beta; running stats (may be NULL) updated with
 * `momentum` and the unbiased variance like torch. */
int l2q_bn_train_fwd(const void* x, const void* gamma, const void* beta, double eps,
                     double momentum, void* running_mean, void* running_var, int M, int N,
                     int elem_bytes, void* y, void* save_mean, void* save_invstd, void* stream);
/* dx overwritten; dgamma, dbeta += */
int l2q_bn_bwd(const void* dy, const void* x, const void* save_mean, const void* save_invstd,
               const void* gamma, int M, int N, int elem_bytes, void* dx, void* dgamma,
               void* dbeta, void* stream);
/* adjoint of l2q_im2col_periodic_f32 (gather form, no atomics): dx (strides sn, sc, sh, sw)
 * overwritten with the sum of the dcol entries that read each input pixel */
int l2q_col2im_periodic_f32(const float* dcol, long sn, long sc, long sh, long sw, int nb, int C,
                            int H, int W, int k, int channels_last_cols, float* dx,
                            void* stream);
int l2q_col2im_periodic_f64(const double* dcol, long sn, long sc, long sh, long sw, int nb, int C,
                            int H, int W, int k, int channels_last_cols, double* dx,
                            void* stream);
/* adjoint of l2q_maxpool_act_nhwc_f32: din[nb][H][W][C] overwritten (first maximum of each
 * window receives dout * act'(out)).  swish is not invertible: it differentiates at the window
 * maximum of `in` (the pre-activation, which the kernel finds anyway); `out` is then not read and
 * may be NULL. */
int l2q_maxpool_act_nhwc_bwd_f32(const float* dout, const float* out, const float* in, int nb,
                                 int H, int W, int C, int pool, int act, float* din,
                                 void* stream);
int l2q_maxpool_act_nhwc_bwd_f64(const double* dout, const double* out, const double* in, int nb,
                                 int H, int W, int C, int pool, int act, double* din,
                                 void* stream);
/* VJP of the U(1) force (the reference differentiates through autograd.grad(create_graph=True),
 * lattice/u1/pytorch/lattice.py:102-117):  dx += D^T [cos(theta) beta (D dF)] */
int l2q_u1_force_bwd(const void* x, const void* dF, double beta, int nb, int T, int X,
                     int elem_bytes, void* dx, void* stream);
/* VJP of the per-chain plaquette sums (action, sin-charge; lattice.py:80-86, 221-224):
 * dx += D^T [-gcos[c] sin(theta) + gsin[c] cos(theta)];  gcos / gsin [nb], either may be NULL */
int l2q_u1_plaq_bwd(const void* x, const void* gcos, const void* gsin, int nb, int T, int X,
                    int elem_bytes, void* dx, void* stream);
/* VJP of l2q_u1_x_update.  x: the field BEFORE the update; gx [nb][n]: cotangent of the
 * updated field; gl [nb] (may be NULL): cotangent of logdet.  dx, ds, dt, dq overwritten,
 * dv +=, deps[c] = per-chain d/d eps (sum over chains on the host side). */
int l2q_u1_x_update_bwd(const void* x, const void* v, const void* s, const void* t, const void* q,
                        const float* mask, int complement, double eps, int forward, int use_ncp,
                        const void* gx, const void* gl, int elem_bytes, int nb, long n, void* dx,
                        void* dv, void* ds, void* dt, void* dq, void* deps, void* stream);
/* VJP of l2q_v_update (real fields).  v: momentum BEFORE the update.  All outputs overwritten. */
int l2q_v_update_bwd(const void* v, const void* force, const void* s, const void* t,
                     const void* q, double eps, int forward, const void* gv, const void* gl,
                     int elem_bytes, int nb, long n, void* dv, void* dF, void* ds, void* dt,
                     void* dq, void* deps, void* stream);
/* VJP of l2q_u1_masked_cos_sin: dx += m (-sin(m x) dout[:, 0:2] + cos(m x) dout[:, 2:4]) */
int l2q_u1_masked_cos_sin_bwd(const void* x, const float* mask, int complement, const void* dout,
                              int nb, long n, int elem_bytes, void* dx, void* stream);
/* torch.optim.Adam step (no weight decay / amsgrad) over one flat parameter arena; the
 * gradient is multiplied by grad_scale first (1/world_size, gradient clipping). step >= 1. */
int l2q_adam(void* p, const void* g, void* m, void* v, long n, double lr, double beta1,
             double beta2, double eps, long step, double grad_scale, int elem_bytes,
             void* stream);
/* out[0] = sum a^2 (gradient norm for clip_grad_norm, trainer.py:1297-1301), order-stable */
int l2q_sumsq(const void* a, long n, int elem_bytes, double* out, void* ws, size_t ws_bytes,
              void* stream);
size_t l2q_sumsq_ws_bytes(long n);

/* ---- SU(3) cotangents (fp64 / complex128, native layout xn[nb][4][9][V]).  Cotangent
 * convention of torch for complex tensors: g_z = dL/dRe z + i dL/dIm z. */

/* VJP of l2q_su3_expm_mul (one masked half-update, dynamics.py:1420-1425 / 1468-1474; eps is
 * the signed step the forward was called with).  gx overwritten, gv +=, deps[c] = per-chain
 * dL/d eps.  Uses the Frechet derivative of the matrix exponential (scaling & squaring). */
int l2q_su3_expm_mul_bwd(const void* xn, const void* vn, double eps, const float* mask_n,
                         int complement, const void* gxnew, void* gx, void* gv, double* deps,
                         int nb, long V, void* ws, size_t ws_bytes, void* stream);
/* VJP of l2q_su3_expm_mul2 (BOTH masked half-updates of a leapfrog step, the mask first or -- complement_first --
 * its complement first; dynamics.py:1420-1425 / 1468-1474 under autograd): the derivative of the matrix
 * exponential is linear in its direction, so the two halves share one exponential and ONE Frechet
 * derivative.  xn: the links BEFORE both halves; gxnew: cotangent of the links after both; same outputs as
 * l2q_su3_expm_mul_bwd (deps = the sum over both halves). */
int l2q_su3_expm_mul2_bwd(const void* xn, const void* vn, double eps, const float* mask_n,
                          int complement_first, const void* gxnew, void* gx, void* gv, double* deps,
                          int nb, long V, void* ws, size_t ws_bytes, void* stream);
/* VJP of l2q_su3_projsu_vec8 (su3_to_vec(projectSU(.)), group.py:138-147): gm += .  `in` are
 * the matrices the forward projected; gvec [nfields][8][V]. */
int l2q_su3_projsu_vec8_bwd(const void* in, const double* gvec, void* gm, long nfields, long V,
                            void* stream);
/* VJP of the force as the reference differentiates it: F = TAH(D x^H) with D = dS/dx held
 * constant (lattice/su3/pytorch/lattice.py:299-308, no create_graph):
 * gx += (beta/3) TAH(gf) (staple sum)^H */
int l2q_su3_force_bwd(const void* xn, const void* gf, double beta, void* gx, int nb, int T, int X,
                      int Y, int Z, void* stream);
/* VJP of the per-plane plaquette sums (action, plaq / charge loss terms, loss.py:56-148):
 * L = sum_planes Re(conj(w[c][p]) sum_sites tr P_p), w [nb][6] complex (re, im), planes ordered
 * as l2q_su3_plaq_planes.  gx += dL/dx. */
int l2q_su3_plaq_bwd(const void* xn, const double* w, void* gx, int nb, int T, int X, int Y, int Z,
                     void* stream);
/* VJP of l2q_su3_wilson_loops: L = sum_{p, c, site} Re(conj(w[p][c][site]) tr P_p(site)), w complex128 laid
 * out like that function's output (torch's cotangent of a complex tensor: dL/dRe + i dL/dIm).  gx += dL/dx. */
int l2q_su3_wilson_loops_bwd(const void* xn, const void* w, void* gx, int nb, int T, int X, int Y, int Z,
                             void* stream);
/* VJP of l2q_su3_clover_reduce: L = sum_c sum_k w[c][k] out[c][k] with out that function's raw [nb][3] output
 * (-sum tr F F, -sum tr(F01 F23 - F02 F13 + F03 F12), sum Re tr P), w [nb][3] real on the device.  gx += dL/dx in
 * the layout and cotangent convention of l2q_su3_plaq_bwd (native [nb][4][9][V] complex128, dL/dRe + i dL/dIm, the
 * links as unconstrained complex 3x3 matrices).  Two gathers, no atomics: pass 1 writes -1/4 (2 w0 F + w1 Fdual) per
 * site and plane into ws, pass 2 has one thread per link collect its 24 inserted loops and 6 staples.  A chain's
 * result is bit-identical alone and in a batch, and from run to run.  Takes any lattice l2q_su3_clover_reduce takes.
 * xn, gx and ws are three different buffers; ws >= nb * 54 * V doubles (432 B per (chain, site)).  Algorithmic
 * traffic: 3168 B per (chain, site) = pass 1 576 (links) + 432 (ws written), pass 2 576 (links) + 432 (ws) + 1152
 * (gx read and written). */
int l2q_su3_clover_bwd(const void* xn, const double* w, void* gx, int nb, int T, int X, int Y, int Z, void* ws,
                       size_t ws_bytes, void* stream);
/* ---- reverse sweep of the Wilson flow (csrc/su3_flow_bwd.hip) */
/* Full VJP of l2q_su3_force, F = (beta/3) TAH(U A(U)): gx += the cotangent of the links for the cotangent gf of F,
 * with the six staples A differentiated as well (l2q_su3_force_bwd holds them constant, as the reference's HMC does;
 * the flow's generator Z(V) = -TAH(V A(V)) needs the whole derivative).  Layout and cotangent convention of
 * l2q_su3_force_bwd / l2q_su3_plaq_bwd (native [nb][4][9][V] complex128, dL/dRe + i dL/dIm, the links as unconstrained
 * complex 3x3 matrices).  With K_l = (beta/3) TAH(gf_l), L = sum_l Re tr(K_l^H U_l A_l): every plaquette occurs four
 * times, once started from each of its links with that link's K inserted, so one thread per link gathers the loops of
 * its 6 plaquettes with 4 insertions each.  No atomics: a chain's result is bit-identical alone and in a batch, and
 * from run to run.  Takes any lattice l2q_su3_force takes.  gx aliases neither xn nor gf.  Algorithmic traffic:
 * 2304 B per (chain, site) = links 576 + gf 576 + gx read and written 1152. */
int l2q_su3_force_vjp(const void* xn, const void* gf, double beta, void* gx, int nb, int T, int X, int Y, int Z,
                      void* stream);
/* Reverse of l2q_su3_flow_stage, P_out = P_in + c TAH(X_in A), X_out = exp(s P_out) X_in, from the stage's input
 * links x_in and its output p_out: gx_in (overwritten) = cotangent of X_in for the cotangent gx_out of X_out; gp is
 * read and written: the cotangent of P_out on entry (what later stages left there), of P_in on exit (P_in enters with
 * weight 1, so it is the same field for a stage without P_in).  Two launches, mirroring the forward: l2q_su3_expm_mul_bwd
 * (its dL/ds goes into ws and is dropped), then l2q_su3_force_vjp at beta = 3 c on gp.  gx_in and gp each alias no
 * other argument; x_in, p_out and gx_out are only read.  ws >= l2q_su3_flow_stage_bwd_ws_bytes. */
size_t l2q_su3_flow_stage_bwd_ws_bytes(int nb, int T, int X, int Y, int Z);
int l2q_su3_flow_stage_bwd(const void* x_in, const void* p_out, double c, double s, const void* gx_out, void* gp,
                           void* gx_in, int nb, int T, int X, int Y, int Z, void* ws, size_t ws_bytes,
                           void* stream);
/* Reverse of one l2q_su3_flow_step of size eps that started from x_in: gx_in (overwritten) = cotangent of x_in for
 * the cotangent gx_out of the step's result.  Recomputes the three stages from x_in with the forward's kernels,
 * keeping P1, P2, P3 apart (the forward overwrites P in place), then reverses the stages 3 -> 1 with the cotangent of
 * P starting at zero.  x_in and gx_out are only read; neither cotangent may alias x_in; gx_in may alias gx_out (gx_out
 * is consumed by stage 3 before gx_in is written by stage 1); ws aliases none of them.
 * ws >= l2q_su3_flow_step_bwd_ws_bytes: seven fields of the links' size (X1, X2, P1, P2, P3, gP, one cotangent; the
 * other cotangent reuses P3) and the stage's scratch, less than eight fields in all. */
size_t l2q_su3_flow_step_bwd_ws_bytes(int nb, int T, int X, int Y, int Z);
int l2q_su3_flow_step_bwd(const void* x_in, double eps, const void* gx_out, void* gx_in, int nb, int T, int X,
                          int Y, int Z, void* ws, size_t ws_bytes, void* stream);
/* ---- improved gauge actions (c1 != 0: Iwasaki / DBW2 rectangles), lattice/su3/pytorch/lattice.py
 * :83-112 (coeffs, _rectangles), :180-196 (rectangle traces of _wilson_loops), :252-269 (action):
 *   S = -(1/3) [ beta (1 - 8 c1) sum_P Re tr P + beta c1 sum_R Re tr R ],  12 planar 2x1 loops R
 * per site.  out[c] = sum_R Re tr R.  ws >= nb * ceil(V / 256) doubles. */
int l2q_su3_rect_reduce(const void* xn, int nb, int T, int X, int Y, int Z, double* out, void* ws,
                        size_t ws_bytes, void* stream);
/* fn += coef * TAH(U (sum of the 18 rectangle staples of the link)): with coef = beta c1 / 3 the
 * rectangle part of grad_action = projectTAH(dS/dx x^H) (lattice.py:299-308) for c1 != 0. */
int l2q_su3_rect_force_add(const void* xn, double coef, void* fn, int nb, int T, int X, int Y, int Z,
                           void* stream);
/* gx += w[c] * d(sum_R Re tr R)/dx  (cotangent of the rectangle term of the action in the
 * Metropolis test of a training step). */
int l2q_su3_rect_bwd(const void* xn, const double* w, void* gx, int nb, int T, int X, int Y, int Z,
                     void* stream);
/* l2q_v_update_bwd for complex128 momenta (SU3): v, force, gv, dv, dF complex [nb][n];
 * s, t, q, ds, dt, dq real [nb][n].  All outputs overwritten. */
int l2q_v_update_bwd_c128(const void* v, const void* force, const double* s, const double* t,
                          const double* q, double eps, int forward, const void* gv,
                          const double* gl, int nb, long n, void* dv, void* dF, double* ds,
                          double* dt, double* dq, double* deps, void* ws, size_t ws_bytes,
                          void* stream);
/* The same VJP with (dF, ds, dt, dq) = this update's cotangents + (acc_dF, acc_ds, acc_dt, acc_dq): the
 * two v-updates either side of a momentum flip or a step boundary act on the same x, hence on ONE force and
 * ONE network evaluation (dynamics.py:1187-1228 with a shared vnet), and the reverse sweep hands the
 * later one's cotangents to the earlier one before the single backward pass through network and force.
 * acc_* may alias nothing that is written. */
int l2q_v_update_bwd_acc_c128(const void* v, const void* force, const double* s, const double* t,
                              const double* q, double eps, int forward, const void* gv, const double* gl,
                              int nb, long n, const void* acc_dF, const double* acc_ds, const double* acc_dt,
                              const double* acc_dq, void* dv, void* dF, double* ds, double* dt, double* dq,
                              double* deps, void* ws, size_t ws_bytes, void* stream);
/* Both v-updates of such a pair reversed in one pass: v_mid = U1(v1) [, v_mid <- -v_mid], v_out = U2(v_mid) with
 * ONE force and ONE (s, t, q); gv = cotangent of v_out.  dv = cotangent of v1; (dF, ds, dt, dq) = the sum of both
 * updates' cotangents; deps1 / deps2 = the per-chain d/d eps of the first / second update.  F, s, t, q are read
 * once (144 instead of 296 bytes per entry for the two calls above).  ws_bytes >= 2 x the single call's. */
int l2q_v_update_bwd_pair_c128(const void* v1, const void* v_mid, const void* force, const double* s,
                               const double* t, const double* q, double eps1, int forward1, double eps2,
                               int forward2, int flip_between, const void* gv, const double* gl, int nb, long n,
                               void* dv, void* dF, double* ds, double* dt, double* dq, double* deps1,
                               double* deps2, void* ws, size_t ws_bytes, void* stream);
/* gx[c][:] += 2 a[c] (x[c][:] - y[c][:]) over n doubles per chain (cotangent of
 * l2q_diff_norm2_reduce, the rmse term of LatticeLoss, loss.py:119-148) */
int l2q_diff_bwd_f64(const double* x, const double* y, const double* a, int nb, long n, double* gx,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* L2Q_H_ */
