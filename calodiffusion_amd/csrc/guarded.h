// The wrapper every C-ABI entry point runs in (the public ABI and its error codes: include/calodiff.h).
#pragma once
#include "../../include/calodiff.h"
#include "cd_common.h"

#include <exception>

namespace cd {

// Every C-ABI entry point runs inside guarded().  The launchers check `hipGetLastError()` after each launch, and that call
// reports the thread's LAST error whoever set it -- a HIP call that failed earlier in the process (another library's, the
// caller's own, or a previous entry point of this one) would otherwise fail the first unrelated launch here (round 3:
// a refused hipEventElapsedTime surfaced as "cd_randn: invalid resource handle").  So the error state is cleared on the way
// in, and again on the way out of a failed call.
template <typename F>
int guarded(F&& f) {
  (void)hipGetLastError();
  try {
    f();
    return CD_OK;
  } catch (const Fail& e) {
    (void)hipGetLastError();
    set_error(e.msg);
    return e.code;
  } catch (const std::exception& e) {
    (void)hipGetLastError();
    set_error(std::string("internal error: ") + e.what());
    return CD_EINVAL;
  }
}

}  // namespace cd

// the entry points are defined at global scope (extern "C") and name the library's own functions unqualified
using namespace cd;
