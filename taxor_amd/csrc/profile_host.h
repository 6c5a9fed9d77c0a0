// profile_host.h -- the host side of a profile's CSR, shared between profile.hip and profile_feed.hip (library-internal).
#pragma once

#include <cstdint>
#include <vector>

// The arrays of a taxor_profile_csr that the host stages of taxor_gpu_profile_run read.  A profile made by
// taxor_gpu_profile_create holds its own; one made by a feed shares the feed's (std::shared_ptr), so the finished CSR is in host
// memory once, whichever of the two objects is destroyed first.
struct taxor_profile_host_csr {
    std::vector<uint64_t> off, ref_len, hash_match, query_len, hash_count;
};
