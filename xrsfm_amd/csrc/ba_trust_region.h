// The Levenberg-Marquardt trust-region rules of Ceres' TrustRegionMinimizer, in one place for every solver of the
// library that uses them: the BA loop (xrsfm_ba.hip: ba_run_impl, 6- and 9-wide), the pose refinement kernel (ba_refine.h:
// k_refine_pose, on lane 0) and the tag refinement (tag_refine.h, host code).  Each caller keeps its own counters, prints and
// exit handling; this holds the radius, the decrease factor and the count of invalid steps in a row.  The expressions are
// written as every site wrote them before, so each site's floating-point results are unchanged.  Plain C++ without HIP.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#define XTR_HD __host__ __device__
#else
#define XTR_HD
#endif

namespace xtr {

constexpr double kMaxRadius = 1e16;
constexpr double kMinRadius = 1e-32;
constexpr double kMinRelDecrease = 1e-3;
constexpr int kMaxInvalidSteps = 5;

// Exit codes (xrsfm_ba_summary::termination_reason): 2 parameter tolerance, 3 function tolerance, 4 minimum radius, 6 invalid steps.
struct TrustRegion {
    double radius;
    double decrease = 2.0;
    int invalid = 0;

    // A step whose model decrease is not positive and finite: 6 on the fifth one in a row (the radius stays), else 0 after the
    // radius shrinks.  A valid step resets the count (invalid = 0).
    XTR_HD int invalid_step() {
        if (++invalid >= kMaxInvalidSteps) return 6;
        radius /= decrease; decrease *= 2.0;
        return 0;
    }
    // Checked on a valid step before the rho test, both keeping the current point: 2, then 3, or 0.
    XTR_HD static int tolerance_exit(double step_norm, double xnorm, double ptol, double cost_change, double cost, double ftol) {
        if (step_norm <= ptol * (xnorm + ptol)) return 2;
        if (std::fabs(cost_change) <= ftol * cost) return 3;
        return 0;
    }
    // rho = actual / model cost decrease
    XTR_HD static bool successful(double rho) { return rho > kMinRelDecrease; }
    XTR_HD void grow(double rho) {
        radius = std::fmin(kMaxRadius, radius / std::fmax(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3)));
        decrease = 2.0;
    }
    // The same rule with the cube written out, for k_lba_resident (ba_lba.h): the inlined pow() cost that kernel a scratch segment.
    // (2 rho - 1)^3 by two multiplications is within an ulp of pow()'s.
    XTR_HD void grow_cubed(double rho) {
        const double x = 2.0 * rho - 1.0;
        radius = std::fmin(kMaxRadius, radius / std::fmax(1.0 / 3.0, 1.0 - x * x * x));
        decrease = 2.0;
    }
    // 4 once the radius is below kMinRadius, else 0
    XTR_HD int shrink() {
        radius /= decrease; decrease *= 2.0;
        return radius < kMinRadius ? 4 : 0;
    }
};

}  // namespace xtr
