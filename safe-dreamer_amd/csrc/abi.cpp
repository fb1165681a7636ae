// ABI version probe of libsdhip.so (see include/sdhip.h).
#include "sdhip.h"

extern "C" int sd_abi_version(void) { return SDHIP_ABI_VERSION; }
