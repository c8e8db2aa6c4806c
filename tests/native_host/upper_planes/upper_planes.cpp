// TEST INFRASTRUCTURE: host driver for the upper-plane form of an anti-Hermitian link field (csrc/su3_math.hpp:
// up_entry, up_plane, m3_from_upper) -- the plane selection of the force kernel's epilogue and the reconstruction
// the projection does in registers -- built for the host under AddressSanitizer + UBSan.
// stdin: one op per line; stdout: one line of numbers per op.
//   planes                -> up_plane(e) for e = 0 .. 8 (9), up_entry(p) for p = 0 .. 5 (6)
//   tah W(9 complex)      -> F = m3_tah(W) (18: re, im per entry) and the matrix rebuilt by m3_from_upper from the six
//                            stored entries of F (18), as hexadecimal bit patterns
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "su3_math.hpp"
using namespace l2q;

static unsigned long long bits(double x) {
  unsigned long long u;
  memcpy(&u, &x, sizeof(u));
  return u;
}

int main() {
  char line[4096];
  while (fgets(line, sizeof(line), stdin)) {
    if (!strncmp(line, "planes", 6)) {
      for (int e = 0; e < 9; ++e) printf("%d ", up_plane(e));
      for (int p = 0; p < 6; ++p) printf("%d ", up_entry(p));
      printf("\n");
    } else if (!strncmp(line, "tah", 3)) {
      M3 w, f, g;
      const char* s = line + 3;
      for (int e = 0; e < 9; ++e) {
        int used = 0;
        if (sscanf(s, "%lf %lf%n", &w.re[e], &w.im[e], &used) != 2) return 2;
        s += used;
      }
      m3_tah(f, w);
      double2 u[6];
      // the epilogue's selection: entry e goes to plane up_plane(e), the three below the diagonal nowhere
      int stored = 0;
      for (int e = 0; e < 9; ++e) {
        const int p = up_plane(e);
        if (p < 0) continue;
        if (p >= 6) return 3;
        u[p] = make_double2(f.re[e], f.im[e]);
        ++stored;
      }
      if (stored != 6) return 4;
      m3_from_upper(g, u);
      for (int e = 0; e < 9; ++e) printf("%llx %llx ", bits(f.re[e]), bits(f.im[e]));
      for (int e = 0; e < 9; ++e) printf("%llx %llx ", bits(g.re[e]), bits(g.im[e]));
      printf("\n");
    } else {
      return 1;
    }
  }
  return 0;
}
