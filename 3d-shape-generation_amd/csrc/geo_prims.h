// Device helpers shared by cloud_geometry.hip and cloud_mesh.hip: the Jacobi eigen-solve of a symmetric 3 x 3 matrix in double.  Contraction
// is off in here, as in the files that include it, and is switched back to the compiler's default at the end.
#pragma once
#include <math.h>

#include "common.h"

namespace pcd {

#pragma clang fp contract(off)

// one Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix, r the third index: app, aqq, apq, arp, arq and the columns p, q of V
__device__ __forceinline__ void geo_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v1p,
                                           double& v2p, double& v0q, double& v1q, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));      // 0 for a theta beyond the range of its square
    const double tn = theta < 0.0 ? -tt : tt;
    const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
    app = app - tn * apq;
    aqq = aqq + tn * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

constexpr int GEO_SWEEPS = 8;      // cyclic Jacobi on 3 x 3 converges quadratically; 5 sweeps reach double precision, the rest are free.
// A sweep is geo_rotate on (0, 1), (0, 2), (1, 2); the callers write the loop out, which keeps their register allocation as it was.

#pragma clang fp contract(fast)

}  // namespace pcd
