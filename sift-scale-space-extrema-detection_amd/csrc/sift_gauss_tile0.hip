// The staged octave-0 instantiations of k_gauss_dog, plain and with the extrema decisions fused.
#include "sift_gauss_tile.h"

namespace sift {

GaussKernelFn gauss_tile0_kernel(int k) {  // kKStaged8, kKStaged16, kKStaged8Fused, kKStaged16Fused
  static const GaussKernelFn f[] = {k_gauss_dog<true, kSW0, 8, false>, k_gauss_dog<true, kSW1, kUR, false>,
                                    k_gauss_dog<true, kSW0, 8, true>, k_gauss_dog<true, kSW1, kUR, true>};
  return f[k - kKStaged8];
}

}  // namespace sift
