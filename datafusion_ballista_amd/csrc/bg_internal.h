/* bg_internal.h — exported symbols of libballista_gpu.so that are NOT
 * public API (kept out of include/ballista_gpu.h): the cross-translation-
 * unit error channel and a test-only hook.  Both translation units include
 * this so a definition that drifts from its declaration fails to compile. */

#ifndef BG_INTERNAL_H
#define BG_INTERNAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* kernels.hip: set the thread-local bg_last_error message; returns code */
int bg_set_error(int code, const char* msg);

/* stage.cpp, test-only: the C++ RecordBatch metadata builder, so CPU tests
 * can pin it byte-for-byte against the Python ipc.py builder.  nodes:
 * (length, null_count) pairs; bufs: (offset, length) pairs.  *out receives
 * malloc'd hex (free with bg_stage_free). */
int bg_debug_rb_message(int64_t n_rows, const int64_t* nodes, int32_t nnodes,
                        const int64_t* bufs, int32_t nbufs, int64_t body_len,
                        int32_t compressed, char** out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* BG_INTERNAL_H */
