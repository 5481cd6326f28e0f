// What the single-launch C entries (for tests; include/innfer_amd.h documents each) share: they upload the small host parameters, call the *_launch function that carries
// the kernel, wait, and free what they uploaded.  An entry makes its refusals BEFORE it constructs an Upload: a refused call touches no device memory.
#pragma once
#include "common.h"

#include <initializer_list>
#include <utility>

namespace innfer {

// host floats -> one device allocation, the parts (pointer, count) one behind the other; freed by the destructor
struct Upload {
    float* d = nullptr;
    int rc = INNFER_OK;
    Upload(const char* what, std::initializer_list<std::pair<const float*, size_t>> parts, const char* items = "parameters") {
        size_t n = 0;
        for (const auto& p : parts) n += p.second;
        if (hipMalloc((void**)&d, (n + 1) * sizeof(float)) != hipSuccess) { d = nullptr; rc = set_error(INNFER_ERR_NOMEM, "%s: out of device memory", what); return; }
        float* q = d;
        for (const auto& p : parts) {
            if (p.second && hipMemcpy(q, p.first, p.second * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { rc = set_error(INNFER_ERR_HIP, "%s: copying the %s failed", what, items); return; }
            q += p.second;
        }
    }
    ~Upload() { if (d) (void)hipFree(d); }
    Upload(const Upload&) = delete;
    Upload& operator=(const Upload&) = delete;
};

// the entry's return: waits for the stream whatever rc is
inline int finish(const char* what, int rc, void* stream) {
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == INNFER_OK) rc = set_error(INNFER_ERR_HIP, "%s: the launch failed", what);
    return rc;
}

}  // namespace innfer
