// em2_csr.h -- a host CSR (toc[0..rowCount], (gene, count) entries) checked and put on the device with toc from 0: the
// host glue of every entry point that reads the expression counts themselves (host only).
#ifndef EM2_CSR_H
#define EM2_CSR_H

#include <vector>

#include "em2_device.h"
#include "em2_hip_util.h"

namespace em2 {

struct UploadedCsr {
    DeviceBuffer toc, data;            // after upload(): toc from 0, the entries toc covers
    std::vector<uint64_t> hostToc;     // after check(): toc from 0
    uint64_t nnz = 0;

    // Host only: toc ascends (where asked) and data is there where toc covers entries.  Returns NULL or the text of the
    // argument error (the caller puts its own name in front).  Reads nothing of a toc without rows.
    const char* check(const uint64_t* tocIn, const CountIn* dataIn, uint32_t rowCount, bool checkAscending = true)
    {
        for (uint32_t r = 0; checkAscending && r < rowCount; ++r) {
            if (tocIn[r] > tocIn[r + 1]) return "toc is not ascending";
        }
        const uint64_t first = rowCount ? tocIn[0] : 0;
        nnz = rowCount ? tocIn[rowCount] - first : 0;
        if (nnz && !dataIn) return "null data";
        hostToc.assign(size_t(rowCount) + 1, 0);
        for (uint32_t r = 0; rowCount && r <= rowCount; ++r) hostToc[r] = tocIn[r] - first;
        source = dataIn ? dataIn + first : nullptr;
        return nullptr;
    }

    // What check() accepted, to the device.
    hipError_t upload()
    {
        EM2_TRY(toc.allocate(hostToc.size() * sizeof(uint64_t)));
        EM2_TRY(data.allocate(nnz * sizeof(CountIn)));
        EM2_TRY(hipMemcpy(toc.p, hostToc.data(), hostToc.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        return nnz ? hipMemcpy(data.p, source, nnz * sizeof(CountIn), hipMemcpyHostToDevice) : hipSuccess;
    }

private:
    const CountIn* source = nullptr;
};

}  // namespace em2

#endif
