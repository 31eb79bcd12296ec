// The two table LMs of the prefix beam search as the library holds them: the character n-gram LM
// (sctc_lm_t) and the lexicon with its word bigrams or word n-grams (sctc_lexicon_t, §4.6,
// §4.6b).
// beam_lm.hip creates and destroys them; ctc_beam.hip reads them into its policies' arguments.
#pragma once
#include "common.h"

struct sctc_lm {
    uint64_t* key = nullptr;   // device [cap]; prob / backoff follow in the same allocation
    float* prob = nullptr;
    float* bo = nullptr;
    int64_t cap = 0;
    int32_t order = 0;
    int32_t bos = 0;
    int device = -1;
};

// The device lexicon of the word-bigram search: the flattened prefix tree (dense child table,
// word id per node), the unigram arrays and an open-addressing table of the listed bigrams.  With a word
// n-gram LM (order != 0) the table holds every listed n-gram of length 2..order under (context id << 32) | w
// and each slot has the n-gram's back-off and its own id as a context next to its value.
struct sctc_lexicon {
    char* mem = nullptr;        // one allocation; the arrays below point into it
    int32_t* child = nullptr;   // [nodes * A]: child node of (node, symbol), -1 for none
    int32_t* word = nullptr;    // [nodes]: word id of the word ending here, -1 for none
    float* ug = nullptr;        // [n_words] unigram value
    float* bo = nullptr;        // [n_words] unigram back-off
    uint64_t* bg_key = nullptr; // [bg_cap] (w1 << 32) | w2, all ones = empty
    float* bg_val = nullptr;    // [bg_cap]
    float* ng_bo = nullptr;     // [bg_cap] n-gram LM only: back-off of the slot's n-gram
    int32_t* ng_id = nullptr;   // [bg_cap] n-gram LM only: its id as a context, -1 at full order
    int64_t nodes = 0, n_words = 0, bg_cap = 0;
    size_t bytes = 0;
    int32_t A = 0, start = 0;
    int32_t order = 0;          // 0: the word-bigram LM of §4.6; 2..5: an n-gram LM of that order
    int32_t space = 0;          // the word separator the tree was checked against
    int device = -1;
};
