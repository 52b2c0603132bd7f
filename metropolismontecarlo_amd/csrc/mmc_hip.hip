// mmc_hip.hip -- single translation unit of libmmc_hip.so (hipcc --offload-arch=gfx950).
// C ABI: include/mmc_hip.h.  No torch types, no CPU fallback: without a HIP device every entry
// point that needs one returns MMC_ERR_HIP.
#include "mmc_host.hpp"
#include "mmc_propose.hpp"

#include "mmc_system.inc"
#include "mmc_ctx.inc"
#include "mmc_batch.inc"
#include "mmc_engine.inc"
#include "mmc_perbox.inc"
#include "mmc_units.inc"
#include "mmc_widom.inc"
#include "mmc_solute.inc"
#include "mmc_deletion.inc"
#include "mmc_forces.inc"
#include "mmc_struct.inc"
#include "mmc_orient.inc"
#include "mmc_pair_energy.inc"
#include "mmc_sofq.inc"
#include "mmc_local.inc"
#include "mmc_cavity.inc"
#include "mmc_vperturb.inc"
#include "mmc_dist.inc"
