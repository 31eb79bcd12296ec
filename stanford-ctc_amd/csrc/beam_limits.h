// Limits and table conventions that the prefix beam search (beam_search.h, beam_policies.h) and the
// handles of its table LMs (beam_lm.hip) both hold to.
#pragma once
#include <stdint.h>

namespace sctc {
namespace beam {

constexpr int AMAX = 256;               // alphabet limit
constexpr int KMAX = 256;               // beam limit
constexpr uint64_t BG_EMPTY = ~0ull;    // an empty slot of the lexicon's bigram or n-gram table
constexpr int NG_MAX_ORDER = 5;         // highest order of the lexicon's word n-gram LM

}  // namespace beam
}  // namespace sctc
