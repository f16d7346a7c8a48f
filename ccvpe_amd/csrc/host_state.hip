// Host state shared by every translation unit of the library: the per-thread error text and the per-device CU count.
#include "common.h"

using namespace ccvpe;

thread_local char ccvpe::g_err[512] = "";

extern "C" const char* ccvpe_last_error(void) { return g_err; }
extern "C" int ccvpe_abi_version(void) { return 7; }

int ccvpe::num_cus() {
  static DevCache cus;                         // per device; 0 = not asked yet
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if ((v = cus.get(dev)) > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
  cus.raise(dev, v);
  return v;
}
