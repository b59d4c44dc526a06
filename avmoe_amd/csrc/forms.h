// The form protocol of a streamed product (DESIGN_CURRENT.md section 3), in one place.  A call site describes its product once (GemmArgs,
// TokPairArgs) and lists the forms that may run it, in order; a form takes (descriptor, stream) and answers 0 = launched, 1 = not served
// (nothing was launched), < 0 = error.  Whether it serves is the form's own business: a call site states no condition that a wrapper states.
#pragma once
#include <hip/hip_runtime.h>

namespace avmoe {

// Tries the forms in order and returns what the first one that does not answer 1 answered (0 or an error); 1 when none served.  A chain
// that ends in launch_gemm (which serves every valid product) never answers 1.
template <class Desc, class... Forms>
int try_forms(Desc& g, hipStream_t st, Forms&&... forms) {
  int rc = 1;
  (void)(... || ((rc = forms(g, st)) <= 0));
  return rc;
}

// A form whose wrapper takes further arguments between the descriptor and the stream (a slab capacity, a second descriptor)
template <class F, class... Extra>
auto with(F f, Extra... extra) {
  return [=](const auto& g, hipStream_t st) { return f(g, extra..., st); };
}

}  // namespace avmoe
