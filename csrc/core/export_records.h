/*
 * libhpnn -- records of a training call handed to the caller: hpnn_batched_stats carries its
 * histories as malloc'ed arrays the caller frees.  Host only (no HIP): the CPU oracle and the GPU
 * driver both use it.
 */
#ifndef HPNN_CORE_EXPORT_RECORDS_H
#define HPNN_CORE_EXPORT_RECORDS_H
#include <libhpnn/ann.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

/* *out = a malloc'ed copy of v (NULL when v is empty), *n = its length; FALSE when malloc failed */
template <typename R>
BOOL export_records(const std::vector<R> &v, R **out, UINT *n) {
    *out = NULL;
    *n = (UINT)v.size();
    if (v.empty()) return TRUE;
    *out = (R *)malloc(v.size() * sizeof(R));
    if (!*out) return FALSE;
    memcpy(*out, v.data(), v.size() * sizeof(R));
    return TRUE;
}
#endif
