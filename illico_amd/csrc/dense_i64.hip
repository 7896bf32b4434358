// dense-input drivers and kernels for int64_t values (u64 keys)
#include "dense_driver.h"
template int run_fused_ovo<int64_t>(illico_ctx *, const FusedCall &, std::vector<u32> &);
template int run_dense_t<int64_t, u64>(illico_ctx *, const void *, int, int64_t, int64_t, int64_t, int64_t, int, int, const OutPlanes &);
template int run_leftovers<int64_t, u64>(illico_ctx *, const void *, int, int64_t, int64_t, int64_t, int64_t, int, int, const OutPlanes &, const u32 *, bool, const int *);
