// The form iter.hip chooses for one genome structure, checked by the compiler (tests/test_cpu_iter_forms.py): compiled host-only
// and syntax-only with -DFL_RTC=1, the directory of the library's own generated flame_spec.h on the include path, and the form
// tests/iter_forms.py expects as -DEXP_RESIDENT=0/1 ... (and -DFL_HOIST_BUDGET=<b> for the fallback budgets).
#include "iter.hip"

static_assert(kSpecResident == (EXP_RESIDENT != 0) && kHoistCol == (EXP_COL != 0) && kHoistAff == (EXP_AFF != 0) &&
              kHoistPost == (EXP_POST != 0) && kHoistFinal == (EXP_FINAL != 0) && kTab == (EXP_TAB != 0) &&
              (kHoistFinal && kSpecPost[FL_SPEC_NXF] != 0) == (EXP_FINAL_POST != 0),
              "iter.hip's form of this structure is not the one tests/iter_forms.py states");
