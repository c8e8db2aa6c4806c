// su3_launch.hpp -- host side of the SU(3) kernels: the argument checks, the t-chunking and the kernel choice that the
// entry points share, and the prototype of every function that one SU(3) .hip defines and another one calls.
#pragma once
#include "su3_links.hpp"

namespace l2q {

inline Dims make_dims(int T, int X, int Y, int Z) { return Dims{T, X, Y, Z, T * X * Y * Z}; }

// positive sizes, and the 36 V complex entries of a chain fit an int (in double: no product of ints can overflow)
inline bool su3_dims_ok(int nb, int T, int X, int Y, int Z) {
  return nb > 0 && T > 0 && X > 0 && Y > 0 && Z > 0 && (double)T * X * Y * Z * 36.0 < 2.0e9;
}
// the same for the per-link entry points, which take n chains or fields of V sites
inline bool su3_field_ok(long n, long V) { return n > 0 && V > 0 && V <= 200000000L; }
// what a checkerboard update needs of the extents
inline bool all_even(int T, int X, int Y, int Z) { return ((T | X | Y | Z) & 1) == 0; }
// a set of directions (bit mu of m): 1..15 with at least two directions; and its size
inline bool dirmask_ok(int m) { return m >= 1 && m <= 15 && (m & (m - 1)) != 0; }
inline int dirmask_count(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }

// Slice-resident kernels sweep t with one workgroup per (chain, spatial tile, t-chunk): the chunks per tile that bring
// `groups` = chains x tiles to about `target` workgroups, at most T, evened out so that no chunk is empty.
// forced > 0 (tuning force_tsplit) replaces the count asked for.
inline int t_chunks(long groups, int T, int target, int forced = 0) {
  long tsplit = forced > 0 ? forced : cdiv(target, groups);
  if (tsplit > T) tsplit = T;
  if (tsplit < 1) tsplit = 1;
  return (int)cdiv(T, cdiv(T, tsplit));
}

// The host side of a slice-resident launch: spatial tiles per chain, t-chunks per tile, workgroups per chain (the
// partial sums a reducing kernel leaves per chain) and the grid size.
struct SliceGrid {
  int nsb, tsplit;
  long per_chain, blocks;
};
inline SliceGrid slice_grid(const Dims& d, int nb, int tile, int target, int forced = 0) {
  const int nsb = d.X * d.Y * d.Z / tile;
  const int tsplit = t_chunks((long)nb * nsb, d.T, target, forced);
  const long per_chain = (long)nsb * tsplit;
  return SliceGrid{nsb, tsplit, per_chain, nb * per_chain};
}
// ... and, once per device, the dynamic LDS that KERN is launched with (su3_force.hip: hipFuncSetAttribute)
void set_dynamic_lds(const void* kern, size_t bytes);
template <auto KERN>
inline void dynamic_lds_once(size_t bytes) {
  static PerDeviceOnce once;
  if (once.first()) set_dynamic_lds((const void*)KERN, bytes);
}

// su3_force_link.hip: the thread-per-link kernel.  A form is the kernel's MODE: Kick is out = vin + coef F (vin ==
// nullptr or out: in place), Vjp is out += coef TAH(vin) A^H (training), the Action forms also store one partial sum
// of Re tr(U A) per workgroup, part[nb][force_link_action_parts], and the Upper forms write the upper-plane field
// [nb][4][6][V] (planes e = 0, 4, 8, 1, 2, 5 of F; the other three are their anti-Hermitian images and are not stored).
enum class LinkForm { Force = 0, Kick = 1, Vjp = 2, ForceAction = 3, Upper = 4, UpperAction = 5 };
bool force_link_applicable(const Dims& d);
int force_link_inmask(const Dims& d);
long force_link_action_parts(const Dims& d, int nb);
// vin: read by Kick and Vjp only; part: written by the Action forms only
void launch_force_link(LinkForm form, const double2* xn, Dims d, int nb, double coef, const double2* vin, double2* out,
                       double* part, hipStream_t st);
// su3_force_plaq.hip: plaquettes shared between their four links (plain force only)
bool force_plaq_applicable(const Dims& d);
void launch_force_plaq(const double2* xn, Dims d, int nb, double coef, double2* out, hipStream_t st);
// su3_flow.hip
bool clover_slice_applicable(const Dims& d);

// su3_force.hip: the force kernel ladder.  Tuning force_tile = 7 (plain force only) the plaquette-sharing kernel, 5
// (the default) and 7 the thread-per-link kernel, where they apply; then the slice-resident kernel where the spatial
// volume is whole tiles, else the LDS-tiled kernel, which takes any lattice.  force_tile = 2 starts at the
// slice-resident kernel (the only way to reach it below the link kernel's size limit).
enum class ForceKernel { PlaqShare, Link, Slice, Tile };
ForceKernel pick_force(const Dims& d, bool kick);
// the thread-per-link family (kick out of place, VJP) runs on this lattice: the kick has no kernel above it
inline bool force_link_runs(const Dims& d) { return pick_force(d, true) == ForceKernel::Link; }
// what l2q_kernel_name (su3_kernels.hip) answers for a force entry point ("": the entry refuses this lattice /
// force_tile); false: `entry` is none of them
bool force_entry_kernel_name(const char* entry, const Dims& d, char* buf, size_t n);

}  // namespace l2q
