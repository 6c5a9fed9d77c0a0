// Stand-in for seqan3's dna5, our own lines: what the reference's syncmer selector (src/hashing/syncmer.cpp) uses
// of it is dna5_vector and dna5::to_char().  TEST INFRASTRUCTURE ONLY.  Assignment from a char keeps A/C/G/T in
// either case (as upper case), maps U/u to T and everything else to N.
#pragma once
#include <vector>

namespace seqan3 {
struct dna5 {
    char c = 'A';
    dna5 &assign_char(char x)
    {
        switch (x) {
        case 'A': case 'a': c = 'A'; break;
        case 'C': case 'c': c = 'C'; break;
        case 'G': case 'g': c = 'G'; break;
        case 'T': case 't': case 'U': case 'u': c = 'T'; break;
        default: c = 'N';
        }
        return *this;
    }
    char to_char() const { return c; }
};
using dna5_vector = std::vector<dna5>;
} // namespace seqan3
