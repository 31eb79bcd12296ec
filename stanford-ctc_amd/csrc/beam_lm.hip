// The handles of the two table LMs of the prefix beam search (beam_lm.h): validation and upload.
// Everything the kernels of ctc_beam.hip follow without a check of their own is checked here, once.
#include <vector>

#include "beam_lm.h"
#include "beam_limits.h"

using namespace sctc;
using namespace sctc::beam;

namespace {

// the sizes of the flattened prefix tree and the id the search starts from
int check_sizes(int64_t nodes, int32_t A, int32_t space, int64_t n_words, int32_t start_word)
{
    SCTC_CHECK_ARG(A >= 2 && A <= AMAX, "lexicon: alphabet size %d outside 2..%d", A, AMAX);
    SCTC_CHECK_ARG(space >= 1 && space < A, "lexicon: space symbol %d outside 1..A-1", space);
    SCTC_CHECK_ARG(nodes >= 1 && nodes <= (int64_t)INT32_MAX / A, "lexicon: %lld nodes outside 1..2^31/A",
                   (long long)nodes);
    SCTC_CHECK_ARG(n_words >= 1 && n_words <= INT32_MAX, "lexicon: %lld words", (long long)n_words);
    SCTC_CHECK_ARG(start_word >= 0 && start_word < n_words, "lexicon: <s> word id %d outside the vocabulary",
                   start_word);
    return SCTC_OK;
}

// the tree itself: everything the lexicon kernels follow in it
int check_tree(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A, int32_t space,
               int64_t n_words)
{
    SCTC_CHECK_ARG(word_host[0] < 0, "lexicon: the root is a word");
    for (int64_t n = 0; n < nodes; ++n) {
        SCTC_CHECK_ARG(word_host[n] >= -1 && word_host[n] < n_words, "lexicon: node %lld has word id %d", (long long)n,
                       word_host[n]);
        SCTC_CHECK_ARG(child_host[n * A] < 0 && child_host[n * A + space] < 0,
                       "lexicon: node %lld has a child for the blank or the space", (long long)n);
        for (int c = 1; c < A; ++c) {
            const int32_t ch = child_host[n * A + c];
            SCTC_CHECK_ARG(ch >= -1 && ch < nodes && ch != 0, "lexicon: node %lld symbol %d -> node %d", (long long)n, c, ch);
        }
    }
    return SCTC_OK;
}

struct LexArray {
    const void* src;
    size_t bytes;
};

// one allocation for all the arrays, each 256-byte aligned; off[i] is where array i went
int upload_lexicon(const LexArray* arr, int n, size_t* off, sctc_lexicon** out)
{
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = total;
        total += align256(arr[i].bytes);
    }
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, total);
    for (int i = 0; i < n && e == hipSuccess; ++i)
        e = hipMemcpy((char*)mem + off[i], arr[i].src, arr[i].bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        return set_error(SCTC_ERR_HIP, "lexicon: upload failed: %s", hipGetErrorString(e));
    }
    sctc_lexicon* lx = new sctc_lexicon();
    lx->mem = (char*)mem;
    lx->bytes = total;
    lx->device = dev;
    *out = lx;
    return SCTC_OK;
}

// the six arrays both kinds of lexicon have, in upload order
void point_lexicon(sctc_lexicon* lx, const size_t* off, int64_t nodes, int64_t n_words, int64_t cap, int32_t A,
                   int32_t start_word)
{
    lx->child = (int32_t*)(lx->mem + off[0]);
    lx->word = (int32_t*)(lx->mem + off[1]);
    lx->ug = (float*)(lx->mem + off[2]);
    lx->bo = (float*)(lx->mem + off[3]);
    lx->bg_key = (uint64_t*)(lx->mem + off[4]);
    lx->bg_val = (float*)(lx->mem + off[5]);
    lx->nodes = nodes;
    lx->n_words = n_words;
    lx->bg_cap = cap;
    lx->A = A;
    lx->start = start_word;
}

}  // namespace

extern "C" {

int sctc_lm_create(const uint64_t* keys_host, const float* prob_host, const float* backoff_host,
                   int64_t capacity, int32_t order, int32_t bos_word, sctc_lm_t* out)
{
    SCTC_CHECK_ARG(out && keys_host && prob_host && backoff_host, "lm: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(capacity >= 2 && (capacity & (capacity - 1)) == 0, "lm: capacity %lld not a power of two",
                   (long long)capacity);
    SCTC_CHECK_ARG(order >= 1 && order <= 8, "lm: order %d outside 1..8", order);
    SCTC_CHECK_ARG(bos_word >= 1 && bos_word <= 255, "lm: <s> word id %d outside 1..255", bos_word);
    int64_t used = 0;
    for (int64_t i = 0; i < capacity; ++i) used += keys_host[i] != 0;
    SCTC_CHECK_ARG(used < capacity, "lm: table without an empty slot");
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    sctc_lm* lm = new sctc_lm();
    const size_t kb = capacity * sizeof(uint64_t), fb = capacity * sizeof(float);
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, kb + 2 * fb);
    if (e == hipSuccess) e = hipMemcpy(mem, keys_host, kb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)mem + kb, prob_host, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)mem + kb + fb, backoff_host, fb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (mem) (void)hipFree(mem);
        delete lm;
        return set_error(SCTC_ERR_HIP, "lm: upload failed: %s", hipGetErrorString(e));
    }
    lm->key = (uint64_t*)mem;
    lm->prob = (float*)((char*)mem + kb);
    lm->bo = (float*)((char*)mem + kb + fb);
    lm->cap = capacity;
    lm->order = order;
    lm->bos = bos_word;
    lm->device = dev;
    *out = lm;
    return SCTC_OK;
}

int sctc_lm_destroy(sctc_lm_t lm)
{
    if (!lm) return SCTC_OK;
    if (lm->key) (void)hipFree(lm->key);
    delete lm;
    return SCTC_OK;
}

int sctc_lexicon_create(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A,
                        int32_t space, const float* ug_prob_host, const float* ug_backoff_host, int64_t n_words,
                        const uint64_t* bg_keys_host, const float* bg_vals_host, int64_t bg_capacity,
                        int32_t start_word, sctc_lexicon_t* out)
{
    SCTC_CHECK_ARG(out, "lexicon: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(child_host && word_host && ug_prob_host && ug_backoff_host && bg_keys_host && bg_vals_host,
                   "lexicon: null argument");
    SCTC_TRY(check_sizes(nodes, A, space, n_words, start_word));
    SCTC_CHECK_ARG(bg_capacity >= 2 && (bg_capacity & (bg_capacity - 1)) == 0,
                   "lexicon: bigram capacity %lld not a power of two", (long long)bg_capacity);
    SCTC_TRY(check_tree(child_host, word_host, nodes, A, space, n_words));
    int64_t used = 0;
    for (int64_t i = 0; i < bg_capacity; ++i) {
        const uint64_t k = bg_keys_host[i];
        if (k == BG_EMPTY) continue;
        ++used;
        SCTC_CHECK_ARG((int64_t)(k >> 32) < n_words && (int64_t)(k & 0xFFFFFFFFull) < n_words,
                       "lexicon: bigram slot %lld names a word outside the vocabulary", (long long)i);
    }
    SCTC_CHECK_ARG(used < bg_capacity, "lexicon: bigram table without an empty slot");
    const LexArray arr[6] = {{child_host, (size_t)nodes * A * sizeof(int32_t)},  {word_host, (size_t)nodes * sizeof(int32_t)},
                             {ug_prob_host, (size_t)n_words * sizeof(float)},    {ug_backoff_host, (size_t)n_words * sizeof(float)},
                             {bg_keys_host, (size_t)bg_capacity * sizeof(uint64_t)},
                             {bg_vals_host, (size_t)bg_capacity * sizeof(float)}};
    size_t off[6];
    sctc_lexicon* lx = nullptr;
    SCTC_TRY(upload_lexicon(arr, 6, off, &lx));
    point_lexicon(lx, off, nodes, n_words, bg_capacity, A, start_word);
    lx->space = space;
    *out = lx;
    return SCTC_OK;
}

int sctc_lexicon_create_ngram(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A,
                              int32_t space, const float* ug_prob_host, const float* ug_backoff_host, int64_t n_words,
                              const uint64_t* ng_keys_host, const float* ng_vals_host, const float* ng_backoffs_host,
                              const int32_t* ng_ids_host, int64_t ng_capacity, int64_t n_contexts, int32_t order,
                              int32_t start_word, sctc_lexicon_t* out)
{
    SCTC_CHECK_ARG(out, "lexicon: null argument");
    *out = nullptr;
    SCTC_CHECK_ARG(child_host && word_host && ug_prob_host && ug_backoff_host && ng_keys_host && ng_vals_host &&
                       ng_backoffs_host && ng_ids_host,
                   "lexicon: null argument");
    SCTC_CHECK_ARG(order >= 2 && order <= NG_MAX_ORDER, "lexicon: n-gram order %d outside 2..%d", order, NG_MAX_ORDER);
    SCTC_TRY(check_sizes(nodes, A, space, n_words, start_word));
    SCTC_CHECK_ARG(ng_capacity >= 2 && (ng_capacity & (ng_capacity - 1)) == 0,
                   "lexicon: n-gram capacity %lld not a power of two", (long long)ng_capacity);
    SCTC_CHECK_ARG(n_contexts >= 0 && n_words + n_contexts <= INT32_MAX, "lexicon: %lld n-gram contexts",
                   (long long)n_contexts);
    SCTC_TRY(check_tree(child_host, word_host, nodes, A, space, n_words));
    // a key is (id of the context << 32) | word; a slot's id is the n-gram's own as a context, -1 at full order
    const int64_t n_ids = n_words + n_contexts;
    int64_t used = 0;
    for (int64_t i = 0; i < ng_capacity; ++i) {
        const uint64_t k = ng_keys_host[i];
        if (k == BG_EMPTY) continue;
        ++used;
        SCTC_CHECK_ARG((int64_t)(k >> 32) < n_ids && (int64_t)(k & 0xFFFFFFFFull) < n_words,
                       "lexicon: n-gram slot %lld names a context or a word outside the table", (long long)i);
        SCTC_CHECK_ARG(ng_ids_host[i] == -1 || (ng_ids_host[i] >= n_words && ng_ids_host[i] < n_ids),
                       "lexicon: n-gram slot %lld has the id %d outside the table", (long long)i, ng_ids_host[i]);
    }
    SCTC_CHECK_ARG(used < ng_capacity, "lexicon: n-gram table without an empty slot");
    // the length of every listed n-gram, through the n-gram its context id names: a context is a word (length 1) or
    // the one listed n-gram with that id; an n-gram has an id exactly when it is shorter than `order`
    std::vector<int8_t> id_len(n_contexts, 0), slot_len(ng_capacity, 0);
    for (int len = 2; len <= order; ++len) {
        for (int64_t i = 0; i < ng_capacity; ++i) {
            if (ng_keys_host[i] == BG_EMPTY || slot_len[i]) continue;
            const int64_t ctx = (int64_t)(ng_keys_host[i] >> 32);
            if ((ctx < n_words ? 1 : id_len[ctx - n_words]) != len - 1) continue;
            slot_len[i] = (int8_t)len;
        }
        for (int64_t i = 0; i < ng_capacity; ++i) {
            if (slot_len[i] != len || ng_ids_host[i] < 0) continue;
            int8_t& l = id_len[ng_ids_host[i] - n_words];
            SCTC_CHECK_ARG(l == 0, "lexicon: n-gram slot %lld has the id %d of another n-gram", (long long)i, ng_ids_host[i]);
            l = (int8_t)len;
        }
    }
    for (int64_t i = 0; i < ng_capacity; ++i) {
        if (ng_keys_host[i] == BG_EMPTY) continue;
        SCTC_CHECK_ARG(slot_len[i], "lexicon: n-gram slot %lld has a context that is no listed n-gram of length < %d",
                       (long long)i, order);
        SCTC_CHECK_ARG((ng_ids_host[i] < 0) == (slot_len[i] == order),
                       "lexicon: n-gram slot %lld of length %d %s an id at order %d", (long long)i, (int)slot_len[i],
                       ng_ids_host[i] < 0 ? "lacks" : "has", order);
    }
    const LexArray arr[8] = {{child_host, (size_t)nodes * A * sizeof(int32_t)},  {word_host, (size_t)nodes * sizeof(int32_t)},
                             {ug_prob_host, (size_t)n_words * sizeof(float)},    {ug_backoff_host, (size_t)n_words * sizeof(float)},
                             {ng_keys_host, (size_t)ng_capacity * sizeof(uint64_t)},
                             {ng_vals_host, (size_t)ng_capacity * sizeof(float)},
                             {ng_backoffs_host, (size_t)ng_capacity * sizeof(float)},
                             {ng_ids_host, (size_t)ng_capacity * sizeof(int32_t)}};
    size_t off[8];
    sctc_lexicon* lx = nullptr;
    SCTC_TRY(upload_lexicon(arr, 8, off, &lx));
    point_lexicon(lx, off, nodes, n_words, ng_capacity, A, start_word);
    lx->space = space;
    lx->ng_bo = (float*)(lx->mem + off[6]);
    lx->ng_id = (int32_t*)(lx->mem + off[7]);
    lx->order = order;
    *out = lx;
    return SCTC_OK;
}

int sctc_lexicon_destroy(sctc_lexicon_t lexicon)
{
    if (!lexicon) return SCTC_OK;
    if (lexicon->mem) (void)hipFree(lexicon->mem);
    delete lexicon;
    return SCTC_OK;
}

size_t sctc_lexicon_bytes(sctc_lexicon_t lexicon) { return lexicon ? lexicon->bytes : 0; }

}  // extern "C"
