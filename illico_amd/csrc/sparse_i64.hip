// CSC / CSR drivers and kernels for int64_t values (u64 keys), int32 and int64 indices
#include "sparse_driver.h"
template int run_sparse_t<int64_t, int32_t, u64>(illico_ctx *, bool, const void *, const void *, const void *, int, int64_t, int64_t, int64_t, int64_t, int, int, const OutPlanes &, SparseAllow);
#ifndef ILLICO_DEV_F32_ONLY
template int run_sparse_t<int64_t, int64_t, u64>(illico_ctx *, bool, const void *, const void *, const void *, int, int64_t, int64_t, int64_t, int64_t, int, int, const OutPlanes &, SparseAllow);
#endif
