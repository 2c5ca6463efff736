// table_packer.hpp -- host vectors on their way into ONE device array: how every plan of the three C ABIs (chain,
// tree, Newton-KKT) puts its tables on its device.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace sipamd {

// Push a vector and name the pointer that is to point at its copy; upload() allocates the array (on the current
// device: the caller holds a DeviceGuard), copies it and sets every such pointer.
template <class T>
struct TablePacker {
  std::vector<T> flat;
  std::vector<std::pair<const T **, size_t>> wanted;
  void push(const std::vector<T> &v, const T **dst = nullptr) {
    if (dst != nullptr)
      wanted.push_back({dst, flat.size()});
    flat.insert(flat.end(), v.begin(), v.end());
  }
  hipError_t upload(void **d_mem) {
    hipError_t e = hipMalloc(d_mem, std::max<size_t>(1, flat.size()) * sizeof(T));
    if (e == hipSuccess)
      e = hipMemcpy(*d_mem, flat.data(), flat.size() * sizeof(T), hipMemcpyHostToDevice);
    for (size_t k = 0; k < wanted.size() && e == hipSuccess; ++k)
      *wanted[k].first = (const T *)*d_mem + wanted[k].second;
    return e;
  }
};

} // namespace sipamd
