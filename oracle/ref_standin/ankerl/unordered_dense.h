// Stand-in for martinus/unordered_dense, our own lines: just what the reference's syncmer selector
// (src/hashing/syncmer.cpp) uses of it, so that its selection logic compiles here.  TEST INFRASTRUCTURE ONLY.
//   * detail::wyhash::hash(uint64_t) is the IDENTITY: the library then reports the selected canonical k-mers
//     themselves, and nothing depends on the un-vendored hash (the oracle's wyhash stays unpinned).
//   * set<K> keeps distinct keys in first-insertion order (insert, begin, end, size).
#pragma once
#include <cstdint>
#include <unordered_set>
#include <vector>

namespace ankerl::unordered_dense {
namespace detail::wyhash {
inline uint64_t hash(uint64_t x) { return x; }
} // namespace detail::wyhash

template <class K> class set {
    std::vector<K> order_;
    std::unordered_set<K> seen_;

public:
    void insert(const K &k)
    {
        if (seen_.insert(k).second) order_.push_back(k);
    }
    typename std::vector<K>::const_iterator begin() const { return order_.begin(); }
    typename std::vector<K>::const_iterator end() const { return order_.end(); }
    size_t size() const { return order_.size(); }
};
} // namespace ankerl::unordered_dense
