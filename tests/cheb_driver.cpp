// CPU driver of tests/test_cheb_ref.py: the scalar recurrence of the Chebyshev preconditioner, dla::cheb_coefficients of
// diaglib_amd/csrc/dla_internal.h, exactly as the HIP engine calls it.  No ROCm include.
//   stdin:   one request per line, "hi lo fac d"
//   stdout:  "theta delta" and then one line "alpha beta gamma eta" per step (d - 1 of them), all as hexadecimal floats
#include <cstdio>
#include "../diaglib_amd/csrc/dla_internal.h"

int main()
{
  double hi, lo, fac;
  int d;
  while (std::scanf("%lf %lf %lf %d", &hi, &lo, &fac, &d) == 4) {
    const dla::ChebCoefficients c = dla::cheb_coefficients(hi, lo, fac, d);
    if ((int)c.steps.size() != (d > 1 ? d - 1 : 0)) return 2;
    std::printf("%a %a\n", c.theta, c.delta);
    for (const dla::ChebStep& s : c.steps) std::printf("%a %a %a %a\n", s.alpha, s.beta, s.gamma, s.eta);
  }
  return 0;
}
