// seg_hist_counters.cpp — TEST INFRASTRUCTURE ONLY.  The counters of kj_core.h's KJ_SEG_HISTO for an emulation library built
// with -DKJ_SEG_HIST (tests/tools/seg_hist.py links this file next to kernel_emu.cpp).
#include <cstring>

namespace kj { unsigned long long kj_seg_hist[4][64]; }

extern "C" void emu_seg_hist(unsigned long long *out, int reset) {
  memcpy(out, kj::kj_seg_hist, sizeof kj::kj_seg_hist);
  if (reset) memset(kj::kj_seg_hist, 0, sizeof kj::kj_seg_hist);
}
