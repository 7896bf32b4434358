// The COOP form of k_ovr_partition_packed (kernels_ovr_partition.h: long blocks dealt over all the wavefronts of a gene's workgroup) in a
// translation unit of its own: the plain form in keyed_u32.hip / keyed_u64.hip keeps the code it had.
#include "keyed_driver.h"

template <typename KeyT>
int launch_ovr_partition_packed_coop(illico_ctx *c, const OvrPartPackedParams &Q, int nb) {
    return launch_kernel(c, k_ovr_partition_packed<KeyT, true>, dim3(nb), dim3(OVRP_NT), ovrp_lds_bytes(), Q);
}
template int launch_ovr_partition_packed_coop<u32>(illico_ctx *, const OvrPartPackedParams &, int);
#ifndef ILLICO_DEV_F32_ONLY
template int launch_ovr_partition_packed_coop<u64>(illico_ctx *, const OvrPartPackedParams &, int);
#endif
