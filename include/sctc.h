/*
 * sctc.h -- C ABI of libsctc_hip.so: the MI355X (gfx950) drop-in for the
 * per-utterance training hot path of amaas/stanford-ctc.
 *
 * Every entry point replaces one interface of the reference (cited per function,
 * paths relative to the reference root).  The reference is Python over (a) a
 * Cython extension `ctc_fast` and (b) the cudamat CUDA library; a maintainer binds
 * this header with ctypes (INTEGRATION.md shows the stubs; the host-side mirror in
 * stanford-ctc_amd/ is exactly that binding).
 *
 * Conventions
 *   - plain C types only; `void* stream` is a hipStream_t (NULL = default stream).
 *   - "dev" pointers are HIP device pointers, "host" pointers ordinary memory.
 *   - the library never allocates device memory: the caller hands in parameter,
 *     gradient and workspace buffers (sizes come from the *_query functions).
 *   - return 0 (SCTC_OK) on success, < 0 on error (sctc_last_error() has the text).
 *     Numerical failure of an utterance (the reference's `skip`, ctc_fast.pyx:147-149)
 *     is reported through skip flags, never through the return code.
 *   - matrices: the reference stores (features x frames) column-major, i.e. one
 *     frame = `features` consecutive floats.  Here that is row-major [frames][ld].
 */
#ifndef SCTC_H_
#define SCTC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCTC_ABI_VERSION 6

#define SCTC_OK 0
#define SCTC_ERR_ARG (-1)       /* bad argument (the reference raises ValueError/AssertionError) */
#define SCTC_ERR_HIP (-2)       /* HIP runtime error */
#define SCTC_ERR_WORKSPACE (-3) /* workspace too small */
#define SCTC_ERR_TIMEOUT (-4)   /* a persistent recurrent launch gave up waiting for its peers (device not
                                   exclusively ours).  The synchronous entry points re-run such a step by
                                   themselves (device lease, then per-step launches) and only report this
                                   when they may not (SCTC_FLAG_ACCUMULATE); sctc_brnn_check reports it for
                                   asynchronous steps */
#define SCTC_ERR_STATE (-5)

#define SCTC_F32 0
#define SCTC_F64 1
#define SCTC_F16 2   /* operand type of the mixed-precision GEMMs / recurrent step (fp32 accumulate) */
#define SCTC_BF16 3
#define SCTC_BF16X3 4 /* fp32 operands split exactly into three bfloat16 terms (x = x1 + x2 + x3), six cross
                         products on the bfloat16 matrix cores, fp32 accumulate: an fp32-accurate GEMM */
#define SCTC_OPERANDS_16BIT 0x100 /* sctc_gemm_h16 only, OR-ed into SCTC_F16 / SCTC_BF16: A_dev and B_dev already
                                     point at 16-bit elements of that type (lda / ldb count them) -- the shadow
                                     copies a producer wrote -- instead of fp32 values to be rounded */

/* ---- library ---------------------------------------------------------- */

int sctc_abi_version(void);
const char* sctc_last_error(void);
/* cm.cuda_set_device(n), runNNet.py:117-120 */
int sctc_set_device(int device);
/* compute units / LDS per CU / total memory of the current device (any may be NULL) */
int sctc_device_info(int* compute_units, int* lds_bytes_per_cu, int64_t* total_mem_bytes,
                     char* name, int name_len);
/* Shared-device mode.  The reference's per-step launches (brnnet.py:148-152, :215-224) work on a
 * GPU that other processes use as well; the persistent recurrent kernels that replace them need
 * every workgroup of a pass resident at once.  With shared-device mode on, each persistent launch
 * runs under an inter-process lease (flock on a per-device file in /dev/shm), synchronously: two
 * ranks on one GPU take turns instead of dead-locking each other.  Initial value: environment
 * variable SCTC_SHARED_DEVICE (the Python mirror sets it when two ranks of a job report the same
 * physical device, sctc_device_pci_bus_id below); switched on automatically, for the rest of the
 * process, by the first SCTC_ERR_TIMEOUT (one line on stderr).  One rank per GPU pays nothing. */
int sctc_set_shared_device(int32_t on);
int sctc_shared_device(void);
/* PCI bus id ("0000:c1:00.0") of HIP device `device` (-1: the current one): the PHYSICAL identity of
 * the GPU, the same string in every process whatever HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES
 * renumbering the launcher applied.  The reference selects its GPU by ordinal (runNNet.py:117-120,
 * cm.cuda_set_device) and never needs to know; the data-parallel ranks exchange this id to find out
 * whether two of them sit on one GPU (stanford-ctc_amd/dist_sgd.py).  Writes a NUL-terminated string. */
int sctc_device_pci_bus_id(int32_t device, char* out, int32_t out_len);

/* ---- CTC: ctc_fast/ctc-loss/ctc_fast.pyx ------------------------------- */

/* Layout of a batch of utterances over the rows of `probs`/`grad`:
 *   rowbase_dev == NULL : utterance b owns rows frame_off[b] .. frame_off[b]+T_b[b]-1
 *                         (frame t = row frame_off[b]+t) -- the reference's (A,T) F-order
 *                         array is exactly one such block with ld == A;
 *   rowbase_dev != NULL : packed time-major minibatch, frame t of utterance b is row
 *                         rowbase_dev[t] + frame_off[b]  (utterances sorted by length,
 *                         frame_off[b] = rank of b; used by the BRNN engine).            */
typedef struct sctc_ctc_batch {
    int32_t B;                 /* utterances */
    int32_t A;                 /* alphabet size incl. blank (params.shape[0], ctc_fast.pyx:24) */
    int32_t blank;             /* blank id (ctc_fast.pyx:14) */
    int32_t dtype;             /* SCTC_F32 | SCTC_F64: type of probs, grad and the lattices */
    int64_t ld;                /* row stride of probs/grad in elements (>= A) */
    const int32_t* T_b;        /* host [B]  frames per utterance  (params.shape[1]) */
    const int32_t* U_b;        /* host [B]  labels per utterance  (seq.shape[0]), >= 1 */
    const int64_t* frame_off;  /* host [B]  see above */
    const int32_t* labels;     /* host, concatenated label ids (seq) */
    const int64_t* label_off;  /* host [B]  first label of utterance b in `labels` */
    const int32_t* rowbase_dev;/* device [max T] or NULL */
} sctc_ctc_batch;

/* bytes of device workspace sctc_ctc_loss_batch needs for this batch (0: the batch is rejected, sctc_last_error()).
 * No bound on the label length or the alphabet (round 5; ctc_fast.pyx:22-32 has none): label rows of up to 512
 * lattice states (2U+1) keep ONE packed half lattice per direction (the alpha / beta / gradient kernel of
 * csrc/ctc_fused.hip), rows of up to 2048 states two float64 lattices of 64 K states per frame
 * (csrc/ctc_kernels.hip), longer rows and alphabets beyond 256 symbols two float64 lattices of round_up(2U+2, 64)
 * states per frame (csrc/ctc_generic.hip). */
size_t sctc_ctc_workspace_bytes(const sctc_ctc_batch* batch);

/* ctc_loss(params, seq, blank) of ctc_fast.pyx:13-152 for B utterances at once.
 *   probs_dev : softmax outputs (the reference's `params`), rows as described above
 *   grad_dev  : d cost / d (pre-softmax activations), same layout as probs (ctc_fast.pyx:138-145);
 *               zeros for utterances with skip != 0
 *   cost_dev  : device double[B], -llForward (ctc_fast.pyx:152); +inf when T is too short
 *               for the label sequence (empty band, log(0))
 *   skip_dev  : device int32[B], 1 where the reference takes its except-branch
 *               (a frame normaliser == 0: infeasible alignment / zero-probability label) */
int sctc_ctc_loss_batch(const sctc_ctc_batch* batch, const void* probs_dev, void* grad_dev,
                        double* cost_dev, int32_t* skip_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream);

/* brnnet.py:161-168 softmax over the alphabet for every frame (row):
 * subtract the row max, exp, scale by 1/sum.  In place allowed. f32 only. */
int sctc_softmax_rows(const float* logits_dev, float* probs_dev, int64_t rows, int32_t A,
                      int64_t ld, void* stream);

/* decode_best_path argmax stage (ctc_fast.pyx:165): per-row argmax over A, first maximum wins */
int sctc_argmax_rows(const void* probs_dev, int32_t dtype, int32_t* best_dev, int64_t rows,
                     int32_t A, int64_t ld, void* stream);

/* ---- decoding: ctc_fast/new_decoder/decoder.pyx BeamLMDecoder -----------
 * Added without an ABI version bump (still 6): sctc_lm_create / sctc_lm_destroy,
 * sctc_ctc_beam_workspace_bytes, sctc_ctc_beam_decode_batch. */

/* A character n-gram LM on the device (stanford-ctc_amd/arpa_lm.py packs it): an open-addressing
 * table of `capacity` slots (a power of two, at least one empty), slot of a key = splitmix64(key) &
 * (capacity-1), then linear probing.  key: the n-gram's word ids (1..255) oldest first, 8 bits each,
 * newest in the low byte (0 = empty slot); prob / backoff: log10 values.  Order <= 8.  The one
 * allocating call of the library: the table lives until sctc_lm_destroy. */
typedef struct sctc_lm* sctc_lm_t;
int sctc_lm_create(const uint64_t* keys_host, const float* prob_host, const float* backoff_host,
                   int64_t capacity, int32_t order, int32_t bos_word, sctc_lm_t* out);
int sctc_lm_destroy(sctc_lm_t lm);

/* BeamLMDecoder.decode(probs, beam, alpha, beta) (decoder.pyx:136-193) for B utterances: CTC prefix
 * beam search over natural-log probabilities (symbol 0 the blank), rows as in sctc_ctc_batch with
 * rowbase_dev == NULL (frame t of utterance b = row frame_off[b] + t, T_b[b] >= 0 frames).  The sort
 * key of a prefix is log(p_nb + p_b) + beta * len, its LM term alpha * log10 P_LM(c | <s> + prefix). */
typedef struct sctc_beam_config {
    int32_t B;                 /* utterances */
    int32_t A;                 /* symbols incl. blank, 2..256 */
    int32_t dtype;             /* SCTC_F32 | SCTC_F64: type of probs */
    int32_t beam;              /* 1..256 */
    int32_t nbest;             /* hypotheses returned per utterance, 1..beam */
    int32_t reserved;          /* 0 */
    int64_t ld;                /* row stride of probs in elements (>= A) */
    const int32_t* T_b;        /* host [B] */
    const int64_t* frame_off;  /* host [B] */
    double alpha;              /* LM weight */
    double beta;               /* length bonus */
    sctc_lm_t lm;              /* NULL: no LM term */
    const int32_t* sym_word;   /* host [A]: LM word id (1..255) of symbols 1..A-1; ignored without LM */
} sctc_beam_config;

/* bytes of device workspace for this batch (0: rejected, sctc_last_error()): per utterance
 * 24 * beam * A bytes (+ 8 * beam * A with an LM) and 4 * beam bytes per frame */
size_t sctc_ctc_beam_workspace_bytes(const sctc_beam_config* cfg);

/* Outputs (device): hypothesis n of utterance b (best first) is ids_dev[nbest * sum(T_b[<b]) + n * T_b[b]
 * + i], i < lengths_dev[b * nbest + n]; scores_dev[b * nbest + n] its sort key (float64).  Fewer than
 * n + 1 prefixes: length 0, score -inf.  ids_dev holds nbest * sum(T_b) int32. */
int sctc_ctc_beam_decode_batch(const sctc_beam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                               int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream);

/* ---- decoding to words: ctc_fast/decoder/bg_decoder.pyx decode_bg_lm -----
 * Added without an ABI version bump (still 6): sctc_lexicon_create / sctc_lexicon_destroy /
 * sctc_lexicon_bytes, sctc_ctc_lexbeam_workspace_bytes, sctc_ctc_lexbeam_decode_batch;
 * sctc_lexicon_create_ngram (§4.6b). */

/* A lexicon on the device (stanford-ctc_amd/decoder/prefixTree.py flattens it): the prefix tree of
 * the word list and the word-bigram LM of fastdecode/lm.cpp.
 *   child_host [nodes * A]  child node of (node, symbol) or -1; node 0 is the root; no node has a
 *                           child for the blank or for `space`, no child is the root
 *   word_host  [nodes]      id of the word that ends at the node or -1; the root is no word
 *   ug_prob_host / ug_backoff_host [n_words]  natural-log unigram value and back-off
 *   bg_keys_host / bg_vals_host [bg_capacity] open addressing, capacity a power of two with at least
 *                           one empty slot: key (w1 << 32) | w2, all ones = empty, slot of a key =
 *                           splitmix64(key) & (capacity-1), then linear probing
 * bg_prob(w1, w2) is the listed value unless that is missing or exactly 0, then the float32 sum
 * ug_backoff[w1] + ug_prob[w2] (lm.cpp:119-127).  start_word: the id of <s>.  Allocates; the
 * lexicon lives until sctc_lexicon_destroy.  Every index the search follows is checked here. */
typedef struct sctc_lexicon* sctc_lexicon_t;
int sctc_lexicon_create(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A,
                        int32_t space, const float* ug_prob_host, const float* ug_backoff_host, int64_t n_words,
                        const uint64_t* bg_keys_host, const float* bg_vals_host, int64_t bg_capacity,
                        int32_t start_word, sctc_lexicon_t* out);

/* The same lexicon with a word n-gram LM of order 2..5 in place of the bigram (DESIGN.md §4.6b;
 * stanford-ctc_amd/decoder/ngram_lm.py packs it).  The tree and the unigram arrays as above, then
 *   ng_keys_host / ng_vals_host / ng_backoffs_host / ng_ids_host [ng_capacity]  every listed n-gram
 *                           w1..wn of length 2..order in one open-addressing table of the same make:
 *                           key (id of w1..w(n-1) << 32) | wn, its natural-log value, its back-off (0
 *                           without one) and its own id, -1 at length `order`
 *   n_contexts              the listed n-grams of length 2..order-1: their ids are n_words ..
 *                           n_words + n_contexts - 1; the id of a unigram is its word id
 * The prefix of every listed n-gram must be listed; its suffix need not be.  P(w | h), h the last
 * order-1 words of <s> and the finished words, is the ARPA back-off rule with float32 partial sums: the
 * value of the longest listed h' w, the match extended one context word at a time and stopped at the
 * first miss, plus the back-offs of the contexts from that length up to h, shortest first, stopped at
 * the first context that is not listed.  A listed value of exactly 0 is a value.  The handle goes to
 * sctc_ctc_lexbeam_workspace_bytes / sctc_ctc_lexbeam_decode_batch like a bigram lexicon, whose LM term
 * then is alpha * P(word | h).  Checked here, before anything is allocated: order 2..5, the tree as above, the
 * capacity, every key's context id and word, and that the ids fit the n-grams -- every context id is a word or the
 * id of exactly one listed n-gram, and an n-gram has an id exactly when it is shorter than `order`.  Values and
 * back-offs are taken as given. */
int sctc_lexicon_create_ngram(const int32_t* child_host, const int32_t* word_host, int64_t nodes, int32_t A,
                              int32_t space, const float* ug_prob_host, const float* ug_backoff_host, int64_t n_words,
                              const uint64_t* ng_keys_host, const float* ng_vals_host, const float* ng_backoffs_host,
                              const int32_t* ng_ids_host, int64_t ng_capacity, int64_t n_contexts, int32_t order,
                              int32_t start_word, sctc_lexicon_t* out);
int sctc_lexicon_destroy(sctc_lexicon_t lexicon);
/* bytes of device memory the lexicon holds (0 for NULL) */
size_t sctc_lexicon_bytes(sctc_lexicon_t lexicon);

/* decode_bg_lm(probs, prefixTree, lm, beam, alpha, beta) for B utterances: the prefix beam search of
 * sctc_ctc_beam_decode_batch in which a prefix may only spell lexicon words separated by `space`, the
 * LM term is alpha * bg_prob(previous word, word) when the space after a word is emitted (alpha * P(word |
 * the last order-1 words) for a lexicon of sctc_lexicon_create_ngram), and the sort key is
 * log(p_nb + p_b) + beta * (words finished). */
typedef struct sctc_lexbeam_config {
    int32_t B;                 /* utterances */
    int32_t A;                 /* symbols incl. blank: the A the lexicon was created with */
    int32_t dtype;             /* SCTC_F32 | SCTC_F64: type of probs */
    int32_t beam;              /* 1..256 */
    int32_t nbest;             /* hypotheses returned per utterance, 1..beam */
    int32_t space;             /* the word separator symbol, 1..A-1 */
    int64_t ld;                /* row stride of probs in elements (>= A) */
    const int32_t* T_b;        /* host [B] */
    const int64_t* frame_off;  /* host [B] */
    double alpha;              /* LM weight */
    double beta;               /* word bonus */
    sctc_lexicon_t lexicon;
} sctc_lexbeam_config;

/* bytes of device workspace (0: rejected, sctc_last_error()): per utterance 24 * beam * A bytes and
 * 4 * beam bytes per frame */
size_t sctc_ctc_lexbeam_workspace_bytes(const sctc_lexbeam_config* cfg);

/* Outputs as sctc_ctc_beam_decode_batch writes them.  After a cut the beam may hold fewer than
 * `beam` prefixes (few words fit): ranks beyond them report length 0 and score -inf. */
int sctc_ctc_lexbeam_decode_batch(const sctc_lexbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream);

/* ---- decoding with a neural character LM: ctc_fast/decoder/clm_decoder2.pyx -----
 * Added without an ABI version bump (still 6): sctc_nnlm_create / sctc_nnlm_destroy / sctc_nnlm_bytes /
 * sctc_nnlm_rows, sctc_ctc_nnbeam_workspace_bytes, sctc_ctc_nnbeam_decode_batch. */

/* A fixed-window feed-forward character LM on the device (stanford-ctc_amd/nn_lm.py holds the model
 * file).  The input is `context` one-hot vectors over `vocab` ids, oldest slot first, so column
 * slot * vocab + id of the first matrix; every hidden layer is relu(W h + b), the output layer is
 * linear and a row is log10 softmax of it.  All float32, the log-softmax in float64.
 *   vocab 3..256, context 1..32, n_layers 2..5 weight matrices (1..4 hidden layers and the output)
 *   widths[n_layers + 1]   widths[0] = context * vocab, widths[n_layers] = vocab, the hidden widths
 *                          between them multiples of 32 up to 2048 (pad with zero units: relu(0) = 0)
 *   weights_host[l]        row-major [widths[l + 1]][widths[l]];  biases_host[l] [widths[l + 1]]
 *   bos_id / null_id       the ids of <s> and <null>: a prefix shorter than the context is preceded
 *                          by <s>, every older slot holds <null> (clm_decoder2.pyx:52-54)
 * The one allocating call: the parameters are repacked and uploaded, and the scratch of
 * sctc_nnlm_rows is part of the handle, which lives until sctc_nnlm_destroy. */
typedef struct sctc_nnlm* sctc_nnlm_t;
int sctc_nnlm_create(int32_t vocab, int32_t context, int32_t n_layers, const int32_t* widths,
                     const float* const* weights_host, const float* const* biases_host, int32_t bos_id,
                     int32_t null_id, sctc_nnlm_t* out);
int sctc_nnlm_destroy(sctc_nnlm_t lm);
/* bytes of device memory the LM holds (0 for NULL) */
size_t sctc_nnlm_bytes(sctc_nnlm_t lm);

/* rows_dev[i * vocab + v] = log10 P(v | contexts_dev[i * context .. + context - 1]) for n contexts of LM
 * ids, oldest first (an id outside 0..vocab-1 is clamped into it).  A row is a function of its context
 * alone, to the bit: not of n, of its position, or of who asks (the search evaluates the same routine).
 * Allocates nothing; calls on one handle share its scratch and must be ordered on one stream. */
int sctc_nnlm_rows(sctc_nnlm_t lm, const int32_t* contexts_dev, int64_t n, float* rows_dev, void* stream);

/* The prefix beam search of sctc_ctc_beam_decode_batch with the LM term alpha * log10 P_NN(c | window of
 * <null>.. <s> prefix).  The fields of sctc_beam_config, the LM handle apart. */
typedef struct sctc_nnbeam_config {
    int32_t B;                 /* utterances */
    int32_t A;                 /* symbols incl. blank, 2..256 */
    int32_t dtype;             /* SCTC_F32 | SCTC_F64: type of probs */
    int32_t beam;              /* 1..256 */
    int32_t nbest;             /* hypotheses returned per utterance, 1..beam */
    int32_t reserved;          /* 0 */
    int64_t ld;                /* row stride of probs in elements (>= A) */
    const int32_t* T_b;        /* host [B] */
    const int64_t* frame_off;  /* host [B] */
    double alpha;              /* LM weight */
    double beta;               /* length bonus */
    sctc_nnlm_t lm;            /* required */
    const int32_t* sym_word;   /* host [A]: LM id (0..vocab-1) of symbols 1..A-1 */
} sctc_nnbeam_config;

/* bytes of device workspace (0: rejected, sctc_last_error()): per utterance what
 * sctc_ctc_beam_workspace_bytes reports with an LM, 64 * beam bytes of context windows and one tile of
 * the LM (256 * widest hidden layer + 128 * (vocab padded to 32) + 128 * context bytes) */
size_t sctc_ctc_nnbeam_workspace_bytes(const sctc_nnbeam_config* cfg);

/* Outputs as sctc_ctc_beam_decode_batch writes them.  Allocates nothing. */
int sctc_ctc_nnbeam_decode_batch(const sctc_nnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                 int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream);

/* ---- decoding with a recurrent character LM: the `rnn` model type of clm_decoder2.pyx -----
 * Added without an ABI version bump (still 6): sctc_rnnlm_create / sctc_rnnlm_destroy / sctc_rnnlm_bytes /
 * sctc_rnnlm_step, sctc_ctc_rnnbeam_workspace_bytes, sctc_ctc_rnnbeam_decode_batch. */

/* A recurrent character LM on the device (stanford-ctc_amd/nn_lm.py, RNNCharLM, holds the model file):
 *   h(empty prefix) = relu(bh + Wx[:, <s>]),  h(P) = relu(bh + Wx[:, id of P's last symbol] + Wh h(P without it)),
 *   row(P) = log10 softmax(Wo h(P) + bo).  All float32, the log-softmax in float64.
 *   vocab 3..256;  hidden a multiple of 32 in 32..2048 (pad with zero units: relu(0) = 0)
 *   Wx [hidden][vocab], Wh [hidden][hidden], Wo [vocab][hidden] row-major, bh [hidden], bo [vocab], on the host
 *   bos_id   the id of <s>, fed into the zero state for the empty prefix
 * The one allocating call: the parameters are repacked and uploaded, and the scratch of sctc_rnnlm_step
 * is part of the handle, which lives until sctc_rnnlm_destroy. */
typedef struct sctc_rnnlm* sctc_rnnlm_t;
int sctc_rnnlm_create(int32_t vocab, int32_t hidden, const float* wx_host, const float* wh_host,
                      const float* bh_host, const float* wo_host, const float* bo_host, int32_t bos_id,
                      sctc_rnnlm_t* out);
int sctc_rnnlm_destroy(sctc_rnnlm_t lm);
/* bytes of device memory the LM holds (0 for NULL) */
size_t sctc_rnnlm_bytes(sctc_rnnlm_t lm);

/* One recurrent step of n independent pairs: state_out_dev[i * hidden ..] = relu(bh + Wx[:, ids_dev[i]] +
 * Wh state_in_dev[i * hidden ..]) and, unless rows_dev is NULL, rows_dev[i * vocab + v] = log10 P(v | that
 * state).  state_in_dev NULL: every input state is zero.  An id outside 0..vocab-1 is clamped into it.  A
 * state and a row are functions of the pair alone, to the bit: not of n, of the pair's position, or of who
 * asks (the search evaluates the same routine).  Allocates nothing; calls on one handle share its scratch
 * and must be ordered on one stream.  The LM must live on the current device. */
int sctc_rnnlm_step(sctc_rnnlm_t lm, const int32_t* ids_dev, const float* state_in_dev, int64_t n,
                    float* state_out_dev, float* rows_dev, void* stream);

/* The prefix beam search of sctc_ctc_beam_decode_batch with the LM term alpha * log10 P_RNN(c | <s> prefix).
 * The fields of sctc_nnbeam_config with the recurrent LM's handle. */
typedef struct sctc_rnnbeam_config {
    int32_t B;                 /* utterances */
    int32_t A;                 /* symbols incl. blank, 2..256 */
    int32_t dtype;             /* SCTC_F32 | SCTC_F64: type of probs */
    int32_t beam;              /* 1..256 */
    int32_t nbest;             /* hypotheses returned per utterance, 1..beam */
    int32_t reserved;          /* 0 */
    int64_t ld;                /* row stride of probs in elements (>= A) */
    const int32_t* T_b;        /* host [B] */
    const int64_t* frame_off;  /* host [B] */
    double alpha;              /* LM weight */
    double beta;               /* length bonus */
    sctc_rnnlm_t lm;           /* required */
    const int32_t* sym_word;   /* host [A]: LM id (0..vocab-1) of symbols 1..A-1 */
} sctc_rnnbeam_config;

/* bytes of device workspace (0: rejected, sctc_last_error()): per utterance what
 * sctc_ctc_beam_workspace_bytes reports with an LM, 8 * beam * hidden bytes of states (two beams) and one
 * tile of the LM (256 * hidden + 128 * (vocab padded to 32) + 512 bytes) */
size_t sctc_ctc_rnnbeam_workspace_bytes(const sctc_rnnbeam_config* cfg);

/* Outputs as sctc_ctc_beam_decode_batch writes them.  Allocates nothing.  The LM must live on the current
 * device.  Diagnostic: with SCTC_RNNBEAM_STATE_COPIES=2..4 in the environment the kernel copies the states of
 * the carried entries that many times per frame instead of once; no result changes, and the time added is a
 * lower estimate of what the copy costs (the repeats find their lines in L2; tools/decode_rnn_bench.py). */
int sctc_ctc_rnnbeam_decode_batch(const sctc_rnnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream);

/* ---- scoring: ctc_fast/editDistance.py, ctc_fast/swbd-utils/editDist.pyx -----
 * Added without an ABI version bump (still 6): sctc_edit_distance_workspace_bytes,
 * sctc_edit_distance_batch. */

/* The Wagner-Fischer table of editDistance.py:14-24 / editDist.pyx:47-58 for P pairs of int32 sequences
 * a (rows, length n) and b (columns, length m): D[i,0] = i, D[0,j] = j, D[i,j] = D[i-1,j-1] where
 * a[i-1] == b[j-1], else 1 + min(D[i-1,j], D[i,j-1], D[i-1,j-1]).  The operation of a cell is the first
 * that holds of MATCH (0: equal symbols), UP (1: D[i-1,j] == D[i,j]-1), LEFT (2: D[i,j-1] == D[i,j]-1),
 * SUB (3) -- the order of the trace-backs, editDistance.py:29-38 and editDist.pyx:71-91.  The path runs
 * from (n,m) along the operations until i == 0 or j == 0; the remaining i count as UP and the remaining
 * j as LEFT (editDistance.py:42-43, editDist.pyx:94-95).
 *   editDistance.edit_distance(ref, hyp): a = ref, b = hyp; ins = UP, dels = LEFT, subs = SUB, corr = MATCH
 *   editDist.edit_distance(hyp, ref):     a = hyp, b = ref; dels = UP, ins = LEFT, subs = SUB, eq = MATCH */
#define SCTC_EDIT_OPS 1   /* also return the path (hyp_corr / ref_corr / errs_by_pos of editDist.pyx:67-106 derive from it) */
typedef struct sctc_edit_config {
    int32_t P;              /* pairs, >= 0 */
    int32_t flags;          /* 0 | SCTC_EDIT_OPS */
    const int32_t* a_len;   /* host [P], 0..8191 */
    const int64_t* a_off;   /* host [P]: pair p's a = a_dev[a_off[p] .. + a_len[p]); offsets may repeat (one
                               reference, many hypotheses) */
    const int32_t* b_len;   /* host [P], 0..8191 */
    const int64_t* b_off;   /* host [P] */
} sctc_edit_config;

/* *bytes: device workspace the batch needs.  0 without SCTC_EDIT_OPS; with it, the 2-bit operation tables
 * of the pairs too large for on-chip memory, about n * m / 4 bytes each. */
int sctc_edit_distance_workspace_bytes(const sctc_edit_config* cfg, size_t* bytes);

/* stats_dev [P][5] int32: D[n,m], UP, LEFT, SUB, MATCH of the path (the return values of
 * editDistance.py:45 in that order).  With SCTC_EDIT_OPS: the operation codes of pair p in FORWARD order
 * (nearest the start of the sequences first, as editDist.pyx:108 reverses its lists) from
 * ops_dev[sum_{q<p} (a_len[q] + b_len[q])], ops_len_dev[p] <= a_len[p] + b_len[p] of them; without it
 * both are NULL.  SCTC_ERR_ARG (no device needed): NULL config, P < 0, a length outside 0..8191, a negative
 * offset, missing output pointers; SCTC_ERR_WORKSPACE: workspace too small.  P == 0 launches nothing.
 * Allocates no device memory; the pair descriptors (40 bytes a pair) go through a pinned host buffer that
 * the calling thread keeps for the life of the process, and the kernel reads them from there.  A call
 * waits for the previous call of the same thread to have read its descriptors, so it cannot be recorded
 * into a stream capture (hipGraph). */
int sctc_edit_distance_batch(const sctc_edit_config* cfg, const int32_t* a_dev, const int32_t* b_dev,
                             int32_t* stats_dev, int8_t* ops_dev, int32_t* ops_len_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);

/* ---- forced alignment and sentence scoring: the align / refScore of ctc_fast/decoder/decoder_utils.py:64-109 -----
 * Added without an ABI version bump (still 6): sctc_ctc_align_workspace_bytes, sctc_ctc_align_batch
 * (DESIGN.md §4.9).  decode() returns (hyp, hypScore, refScore, align); the reference never computed refScore
 * (decoder_utils.py:68-70) and has an alignment for the pointwise-argmax decoder only, so its CTM writer gives
 * every word the whole segment's time (swbd-utils/convert_to_ctm.py:27-37). */

/* Input: natural-log probabilities of a packed batch, [sum T][ld], float32 or float64 (the decoders' layout),
 * -inf allowed; utterance b has T_b[b] rows from row frame_off[b] and the label row l[0..U) =
 * labels_dev[label_off[b] .. + U_b[b]).  Extended row x[s], s = 0..2U (S = 2U+1): x[2u+1] = l[u], even s the
 * blank (ctc_fast.pyx:42-76).  All arithmetic is float64; float32 inputs are widened exactly.
 *   v_0(0) = y_0(blank), v_0(1) = y_0(x[1]), the other states -inf;
 *   v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s odd and x[s] != x[s-2]) + y_t(x[s]),  t >= 1;
 * best takes the largest value, on ties the FIRST of (stay, s-1, s-2); all candidates -inf: -inf, back-pointer
 * "stay".  The path ends in state S-1 unless v_{T-1}(S-2) is STRICTLY larger.  The Viterbi score is that end
 * value, a plain chain of float64 additions.  With SCTC_ALIGN_TOTAL the same pass computes a_t(s) with the
 * max-shifted log-sum-exp in place of best (-inf (+) -inf = -inf, never NaN); the total is
 * a_{T-1}(S-1) (+) a_{T-1}(S-2) = log P_ctc(l | y).
 * status: 0 aligned; 1 no alignment of finite score (T < U + repeats, a lattice cut by -inf): scores -inf,
 * every frame_label and span -1; 2 a label outside [0, A) or equal to the blank: outputs as for 1, nothing
 * outside the row is read.  T = 0: status 0 with scores 0.0 when U = 0, else status 1. */
#define SCTC_ALIGN_TOTAL 1   /* also the sum over all alignments */
typedef struct sctc_align_config {
    int32_t B;              /* utterances, >= 0 */
    int32_t A;              /* symbols, >= 1 */
    int32_t dtype;          /* SCTC_F32 | SCTC_F64 */
    int32_t blank;          /* in [0, A) */
    int32_t ld;             /* elements between rows, >= A */
    int32_t flags;          /* 0 | SCTC_ALIGN_TOTAL */
    const int32_t* T_b;     /* host [B], >= 0 */
    const int64_t* frame_off;   /* host [B] */
    const int32_t* U_b;     /* host [B], 0..4095 */
    const int64_t* label_off;   /* host [B]; offsets may repeat */
} sctc_align_config;

/* *bytes: device workspace the batch needs: the 2-bit back-pointers of the utterances too long for on-chip
 * memory, about T * (2U+1) / 4 bytes each (states rounded up to the launch's width). */
int sctc_ctc_align_workspace_bytes(const sctc_align_config* cfg, size_t* bytes);

/* frame_label_dev int32 [sum T], at frame_off[b]: the index u of the label a frame is aligned to, -1 for blank.
 * span_dev int32 [sum U][2], utterance b at sum_{q<b} U_b[q]: first and last frame of label u, inclusive.
 * scores_dev double [B][2]: Viterbi and total (NaN without SCTC_ALIGN_TOTAL).  status_dev int32 [B].
 * SCTC_ERR_ARG (no device needed): NULL config or outputs, negative sizes, ld < A, a blank outside [0, A),
 * U > 4095, negative offsets, unknown dtype or flags; SCTC_ERR_WORKSPACE: workspace too small.  B == 0 launches
 * nothing.  Allocates no device memory; the utterance descriptors go through the calling thread's pinned host
 * buffer as those of sctc_edit_distance_batch do (same remark on stream capture).  SCTC_ALIGN_PATH=wave|wide in
 * the environment forces the kernel (tests, A/B runs); by default the longest label row decides. */
int sctc_ctc_align_batch(const sctc_align_config* cfg, const void* logprobs_dev, const int32_t* labels_dev,
                         int32_t* frame_label_dev, int32_t* span_dev, double* scores_dev, int32_t* status_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- best-path decoding of a batch: ctc_fast.pyx:154-187 and new_decoder/decoder.pyx:79-100 -------------------
 * Added without an ABI version bump (still 6): sctc_ctc_bestpath_batch, sctc_log_rows.
 *
 * Input: a packed batch [sum T][ld], float32 or float64 (probabilities or log-probabilities: only their order and
 * their sum matter); utterance b has T_b[b] rows from row frame_off[b].
 *   best[t]  the column of the FIRST maximum of row t: `v > bv` from -inf over columns 0..A-1, a row of only -inf
 *            gives 0 -- exactly sctc_argmax_rows.  NaN is outside the contract, as it is there.
 *   frame t emits best[t] iff (t == 0 or best[t] != best[t-1]) and best[t] is none of drop[0..n_drop).  The
 *            comparison is on RAW neighbours: a dropped symbol still separates two runs of one symbol.
 *            ctc_fast.pyx:168-187 is this with drop = {blank, 1, 2, 8}; decoder.pyx:90-98 with drop = {0}.
 * Output: the k-th emitted label of utterance b at ids_dev[o_b + k], o_b = sum_{q<b} T_b[q] (the layout of the beam
 * searches at nbest == 1); lens_dev[b] the number of labels; spans_dev[o_b + k] = (first, last) frame of the label's
 * run of equal best, inclusive (last is the reference's `align`); scores_dev[b] = sum_t row_t[best[t]] in float64,
 * summed in the kernel's order (bit-defined only where every order is exact).  T_b = 0: length 0, score 0.0. */
typedef struct sctc_bestpath_config {
    int32_t B, A, dtype;          /* utterances >= 0, alphabet >= 1, SCTC_F32 | SCTC_F64 */
    int32_t n_drop;               /* 0..16 */
    int32_t drop[16];             /* symbol ids that are never emitted (the blank, the reference's 1, 2, 8, ...) */
    int64_t ld;                   /* row stride in elements, >= A */
    const int32_t* T_b;           /* host [B], >= 0 */
    const int64_t* frame_off;     /* host [B]: first row of utterance b */
} sctc_bestpath_config;

/* ids_dev int32 [sum T], lens_dev int32 [B], spans_dev int32 [sum T][2] or NULL, scores_dev double [B] or NULL.
 * SCTC_ERR_ARG (no device needed): NULL config, ids or lens; B < 0; A < 1; ld < A; n_drop outside 0..16; a negative
 * T_b or frame_off; a dtype other than the two.  B == 0 launches nothing.  One launch, one workgroup per utterance;
 * allocates no device memory; the utterance descriptors go through the calling thread's pinned host buffer as those
 * of sctc_edit_distance_batch do (same remark on stream capture).  SCTC_BESTPATH_MAP=lane|wave in the environment
 * forces the row-to-lane mapping (tests, A/B runs); by default A <= 4096 takes a row per lane, larger A a row per wave. */
int sctc_ctc_bestpath_batch(const sctc_bestpath_config* cfg, const void* rows_dev, int32_t* ids_dev, int32_t* lens_dev,
                            int32_t* spans_dev, double* scores_dev, void* stream);

/* logp = (float) log((double) p), element by element over [rows][A] with row stride ld (columns A..ld are not
 * touched); in place (logp_dev == probs_dev) is allowed; p == 0 gives -inf.  What writeLikelihoods.py computes on
 * the host, for probabilities that stay on the device.  SCTC_ERR_ARG: rows < 0, A < 1, ld < A, a NULL pointer with
 * rows > 0. */
int sctc_log_rows(const float* probs_dev, float* logp_dev, int64_t rows, int32_t A, int64_t ld, void* stream);

/* ---- LM scores of label sequences and n-best rescoring: the second pass (ctc_fast/clm/clm_pp.py, the refScore of
 * decoder_utils.decode) -----
 * Added without an ABI version bump (still 6): sctc_lm_score_workspace_bytes, sctc_lm_score_batch,
 * sctc_nbest_rank_batch. */

#define SCTC_LM_NGRAM 0   /* lm is an sctc_lm_t */
#define SCTC_LM_NN 1      /* an sctc_nnlm_t */
#define SCTC_LM_RNN 2     /* an sctc_rnnlm_t */

/* N sequences of CTC symbol ids on the device: sequence n is l[0..U) = labels_dev[label_off[n] .. + U_b[n]); offsets
 * may repeat and may point into the ids of a beam search in place.  Term i of a sequence is log10 P_LM(l_i | <s>,
 * l_0 .. l_{i-1}) over the LM ids sym_word[l_.]: the float32 value that the beam search of that LM adds for the
 * extension (the same rnnlm_tile / nnlm_tile call, the same table probe and float32 additions). */
typedef struct sctc_lm_score_config {
    int32_t N;                  /* sequences, >= 0 */
    int32_t A;                  /* symbols incl. the blank 0, 1..256 */
    int32_t lm_kind;            /* SCTC_LM_NGRAM | SCTC_LM_NN | SCTC_LM_RNN */
    int32_t reserved;           /* 0 */
    const void* lm;             /* the handle of that kind */
    const int32_t* sym_word;    /* host [A]: LM id of symbols 1..A-1 (n-gram: 1..255; neural: 0..V-1) */
    const int32_t* U_b;         /* host [N], 0..8191 */
    const int64_t* label_off;   /* host [N], >= 0 */
} sctc_lm_score_config;

/* *bytes: device workspace of the call: 24 bytes a sequence, the symbol map, for the recurrent LM 16 bytes per tile of
 * 32 sequences, sum U float32 when `without_terms` (the call gets terms_dev == NULL), and the scratch of at most 512
 * resident tiles of a neural LM; every slice rounded up to 256 bytes (csrc/lm_score_plan.h). */
int sctc_lm_score_workspace_bytes(const sctc_lm_score_config* cfg, int32_t without_terms, size_t* bytes);

/* terms_dev float32 [sum U] or NULL: the terms of sequence n from sum_{q<n} U_b[q].  sums_dev double [N]: the float64
 * sum of the sequence's float32 terms, added in position order; no end-of-sentence term; U = 0 gives 0.0.
 * status_dev int32 [N]: 0, or 2 for a sequence with a label outside [0, A) or equal to 0 (the blank has no LM id):
 * sum -inf, its terms are not written, nothing outside the tables is read.
 * SCTC_ERR_ARG (no device needed): NULL config, handle, arrays or outputs, N < 0, A outside 1..256, an unknown
 * lm_kind, a length outside 0..8191, a negative offset, an LM id outside the LM's range; SCTC_ERR_WORKSPACE:
 * workspace too small.  N == 0 launches nothing.  Allocates no device memory; the descriptors go through the calling
 * thread's pinned host buffer into the workspace (same remark on stream capture as sctc_edit_distance_batch). */
int sctc_lm_score_batch(const sctc_lm_score_config* cfg, const int32_t* labels_dev, float* terms_dev, double* sums_dev,
                        int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Combine and rank B utterances x K hypotheses (K <= 256), pair (b, k) at b * K + k: scores_dev [B * K][2] and
 * status_dev [B * K] of ONE sctc_ctc_align_batch call with SCTC_ALIGN_TOTAL over the pairs, lm_sums_dev [B * K] of
 * sctc_lm_score_batch (NULL: no LM term, the sum counts as 0.0), U_b host [B * K] the lengths, K_b host [B]: the
 * first K_b[b] ranks of utterance b are real hypotheses.  first_scores_dev (double [B * K] or NULL): the first
 * pass's own scores; a rank at -inf there (the searches fill the ranks beyond the beam so) and every rank after it
 * is not real either.
 *   rescored_dev double [B][K]: (total + alpha * lm) + beta * U in float64, no contraction, for a real hypothesis
 *                with align status 0; otherwise -inf.
 *   order_dev int32 [B][K]: the hypothesis indices by descending rescored value, ties to the lower first-pass rank;
 *                the ranks that are not real come last, in their original order.
 * SCTC_ERR_ARG (no device needed): B < 0, K outside 1..256, NULL arrays, K_b outside [0, K], a negative length.
 * B == 0 launches nothing.  One wave per utterance; the lengths go through the calling thread's pinned host buffer. */
int sctc_nbest_rank_batch(int32_t B, int32_t K, const int32_t* K_b, const int32_t* U_b, double alpha, double beta,
                          const double* scores_dev, const int32_t* status_dev, const double* lm_sums_dev,
                          const double* first_scores_dev, double* rescored_dev, int32_t* order_dev, void* stream);

/* ---- word-LM scores of label sequences: the word LM as a second pass -----
 * Added without an ABI version bump (still 6): sctc_word_lm_score_workspace_bytes, sctc_word_lm_score_batch,
 * sctc_nbest_rank_words_batch. */

#define SCTC_WORD_LM_EOS 1            /* one more term, P(</s> | history); not counted as a word */
#define SCTC_WORD_LM_NO_FINAL_WORD 2  /* a last token that no space follows is no word: the lexicon search's count */

/* N sequences of CTC symbol ids on the device, as for sctc_lm_score_batch: sequence n is l[0..U) = labels_dev[
 * label_off[n] .. + U_b[n]); offsets may repeat and may point into the ids of a beam search in place.
 *   tokens   a token is a maximal run of symbols other than the lexicon's space; leading, trailing and repeated
 *            spaces make no empty word (str.split()).  Every token is a word, except the last one when no space
 *            follows it and SCTC_WORD_LM_NO_FINAL_WORD is set.
 *   word id  walk the lexicon's tree from the root over the token's symbols: if every step exists and a word ends at
 *            the last node, that word's id; otherwise the token is out of vocabulary (OOV) and gets `unk`.
 *   term k   the float32 value that the lexicon search adds at the space after word k: bg_prob(previous word, w) of a
 *            bigram lexicon (previous word of word 0: <s>), P(w | the last order-1 words of <s> and the words before)
 *            of an n-gram lexicon; the same device routines, the same bits.  Natural log, the word LM's own unit
 *            (the character LMs' terms are log10).  With SCTC_WORD_LM_EOS one last term, P(</s> | history). */
typedef struct sctc_word_lm_score_config {
    int32_t N;                  /* sequences, >= 0 */
    int32_t A;                  /* symbols incl. the blank 0: the A the lexicon was created with */
    sctc_lexicon_t lexicon;     /* of sctc_lexicon_create or sctc_lexicon_create_ngram */
    int32_t unk;                /* word id of <UNK>, or -1: an OOV word then gives status 3 */
    int32_t end;                /* word id of </s>, or -1 (SCTC_WORD_LM_EOS needs it) */
    int32_t flags;              /* SCTC_WORD_LM_* */
    int32_t reserved;           /* not read */
    const int32_t* U_b;         /* host [N], 0..8191 */
    const int64_t* label_off;   /* host [N], >= 0 */
} sctc_word_lm_score_config;

/* *bytes: device workspace of the call: 24 bytes a sequence and an int32 per slot (below), each slice rounded up to
 * 256 bytes. */
int sctc_word_lm_score_workspace_bytes(const sctc_word_lm_score_config* cfg, size_t* bytes);

/* Sequence n owns the slots from sum_{q<n} (ceil(U_b[q] / 2) + 1): a row of U symbols has at most ceil(U / 2) words,
 * and one slot more for </s>.  terms_dev float32 / word_ids_dev int32 [slots] or NULL: term k and the id of word k
 * (unk for an OOV word, `end` at the </s> term) at slot k of the sequence; the slots past its terms are not written.
 * sums_dev double [N]: the float64 sum of the sequence's terms, added in word order; no words gives 0.0, or the </s>
 * term alone.  counts_dev int32 [N][2]: words, OOV words.  status_dev int32 [N]: 0; 2 for a sequence with a label
 * outside [1, A): sum -inf, counts 0, nothing outside the tables is read; 3 for an OOV word with unk == -1: sum -inf.
 * Terms and word ids of a sequence whose status is not 0 are not written.
 * SCTC_ERR_ARG (no device needed): NULL config, lexicon, arrays or outputs, N < 0, A outside 1..256 or not the
 * lexicon's, unknown flags, unk or end outside -1..words-1, SCTC_WORD_LM_EOS with end == -1, a length outside
 * 0..8191, a negative offset; SCTC_ERR_WORKSPACE: workspace too small.  N == 0 launches nothing.  One launch, one
 * wave per sequence; no atomics: deterministic bit for bit.  Allocates no device memory; the descriptors go through
 * the calling thread's pinned host buffer into the workspace (same remark on stream capture as
 * sctc_edit_distance_batch). */
int sctc_word_lm_score_batch(const sctc_word_lm_score_config* cfg, const int32_t* labels_dev, float* terms_dev,
                             int32_t* word_ids_dev, double* sums_dev, int32_t* counts_dev, int32_t* status_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* sctc_nbest_rank_batch with a word-LM term: word_sums_dev double [B * K], word_counts_dev int32 [B * K][2] and
 * word_status_dev int32 [B * K] of sctc_word_lm_score_batch over the pairs.  A real hypothesis with align status 0 and
 * word status 0 scores, left to right in float64 without contraction,
 *   ((total + alpha * lm) + beta * U) + (word_alpha * word_sum + word_beta * words)
 * any other -inf (no 0 * -inf is formed).  Order, ties, K_b and first_scores_dev as in sctc_nbest_rank_batch, whose
 * kernel this instantiates a second time.  SCTC_ERR_ARG as there, and for a NULL word array. */
int sctc_nbest_rank_words_batch(int32_t B, int32_t K, const int32_t* K_b, const int32_t* U_b, double alpha, double beta,
                                const double* scores_dev, const int32_t* status_dev, const double* lm_sums_dev,
                                const double* first_scores_dev, const double* word_sums_dev,
                                const int32_t* word_counts_dev, const int32_t* word_status_dev, double word_alpha,
                                double word_beta, double* rescored_dev, int32_t* order_dev, void* stream);

/* ---- word interning, minimum Bayes risk selection and word confidences over n-best lists -----
 * Added without an ABI version bump (still 6): sctc_intern_words_workspace_bytes, sctc_intern_words_batch,
 * sctc_nbest_mbr_workspace_bytes, sctc_nbest_mbr_batch. */

/* N rows of CTC symbol ids on the device, as for sctc_lm_score_batch: row n is l[0..U) = labels_dev[label_off[n] .. +
 * U_b[n]); offsets may repeat and may point into the ids of a beam search in place.  group_off cuts the rows into G
 * groups of consecutive rows: group g is rows group_off[g] .. group_off[g + 1] - 1.
 *   tokens   a token is a maximal run of symbols other than `space`; leading, trailing and repeated spaces make no
 *            empty word (str.split(), the rule of sctc_word_lm_score_batch).
 *   ids      number the tokens of a group 0..W-1 in (row, position) order.  The id of token t is the smallest t' <= t
 *            whose token is the same run of symbols: same length, same symbols.  Two tokens of a group have the same id
 *            exactly when they are the same word; no lexicon is involved and a hash never merges two words. */
typedef struct sctc_intern_config {
    int32_t N;                  /* rows, >= 0 */
    int32_t G;                  /* groups, >= 0 */
    int32_t A;                  /* symbols incl. the blank 0, 1..256 */
    int32_t space;              /* the space symbol, in [1, A) */
    const int32_t* U_b;         /* host [N], 0..4095 */
    const int64_t* label_off;   /* host [N], >= 0 */
    const int32_t* group_off;   /* host [G + 1], from 0 to N, never decreasing */
} sctc_intern_config;

/* *bytes: device workspace of the call: 32 bytes a row, 8 bytes a group, 4 bytes a row, 24 bytes a word slot and the
 * groups' hash tables (4 bytes an entry, a power of two of at least twice the group's slots), each slice rounded up to
 * 256 bytes. */
int sctc_intern_words_workspace_bytes(const sctc_intern_config* cfg, size_t* bytes);

/* Row n owns the slots from sum_{q<n} ceil(U_b[q] / 2): a row of U symbols has at most ceil(U / 2) words.
 * word_ids_dev int32 [slots]: the id of word k of the row at its slot k; the slots past its words are not written.
 * counts_dev int32 [N]: the words of the row.  status_dev int32 [N]: 0, or 2 for a row with a label outside [1, A):
 * such a row has count 0, none of its slots is written and nothing outside the row is read.
 * SCTC_ERR_ARG (no device needed): NULL config, arrays or outputs, N < 0, G < 0, A outside 1..256, space outside
 * [1, A), a length outside 0..4095, a negative offset, a group_off that decreases or does not run from 0 to N;
 * SCTC_ERR_WORKSPACE: workspace too small.  N == 0 launches nothing.  The insertion uses atomics on the group's
 * table, of which only an order-independent minimum is kept: the ids are the same bit for bit from run to run.
 * Allocates no device memory; the descriptors go through the calling thread's pinned host buffer into the workspace:
 * a call waits for the previous call of the same thread to have read its descriptors, so it cannot be recorded into a
 * stream capture (hipGraph), as sctc_edit_distance_batch. */
int sctc_intern_words_batch(const sctc_intern_config* cfg, const int32_t* labels_dev, int32_t* word_ids_dev,
                            int32_t* counts_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                            void* stream);

#define SCTC_MBR_CHARS 0  /* the unit of the edit distance is the symbol */
#define SCTC_MBR_WORDS 1  /* the word: the K rows of an utterance are interned as one group */
#define SCTC_MBR_CONF 1   /* also the confidence of every unit of the chosen hypothesis */
#define SCTC_MBR_DIST 2   /* keep the pairwise distances as an output */

/* B utterances x K hypotheses (K <= 256), pair (b, k) at b * K + k, the rows as for sctc_nbest_rank_batch.
 * Hypothesis k of utterance b is REAL when k < K_b[b] and scores_dev[b * K + k] is finite.  In word unit a real row
 * with a label outside [1, A) counts as a row without words. */
typedef struct sctc_mbr_config {
    int32_t B;                  /* utterances, >= 0 */
    int32_t K;                  /* hypotheses per utterance, 1..256 */
    int32_t unit;               /* SCTC_MBR_CHARS | SCTC_MBR_WORDS */
    int32_t flags;              /* 0 | SCTC_MBR_CONF | SCTC_MBR_DIST */
    int32_t A;                  /* symbols incl. the blank 0, 1..256 */
    int32_t space;              /* the space symbol, in [1, A); read in word unit only */
    double scale;               /* finite, >= 0: multiplies the score differences */
    const int32_t* K_b;         /* host [B], 0..K */
    const int32_t* U_b;         /* host [B * K], 0..4095 */
    const int64_t* label_off;   /* host [B * K], >= 0 */
} sctc_mbr_config;

/* *bytes: device workspace of the call (csrc/nbest_mbr_plan.h has the slices): the O(B * K) descriptors, in word unit
 * the interning's workspace and ids, the B * K * K int32 distances unless SCTC_MBR_DIST, with SCTC_MBR_CONF the paths,
 * match flags and the operation tables that do not fit on chip. */
int sctc_nbest_mbr_workspace_bytes(const sctc_mbr_config* cfg, size_t* bytes);

/* scores_dev double [B][K]: the rescored values of sctc_nbest_rank_batch, or the first pass's.  order_dev int32
 * [B][K]: the ranking of sctc_nbest_rank_batch, or NULL.
 *   D        dist_dev int32 [B][K][K] (with SCTC_MBR_DIST; otherwise NULL and D lives in the workspace): D[b][k][j] is
 *            the edit distance (the table of sctc_edit_distance_batch) between hypotheses k and j in the unit, 0 on the
 *            diagonal, -1 where k or j is not real.  One wave per unordered pair of real hypotheses; the host passes
 *            no descriptor per pair.
 *   weights  s_max = the maximum score of the real hypotheses; w_k = exp(scale * (s_k - s_max)), and exactly 1.0
 *            where s_k == s_max; Z = sum_k w_k over the real ranks in ascending k.  All float64, no contraction.
 *   post_dev double [B][K]: w_k / Z, 0 for a rank that is not real.
 *   risk_dev double [B][K]: (sum_j w_j * D[b][k][j], ascending j over the real ranks) / Z, +inf for a rank that is
 *            not real.
 *   best_dev int32 [B]: the real rank of least risk; ties go to the hypothesis that comes first in order_dev[b], with
 *            order_dev == NULL to the lower k; -1 without a real hypothesis.
 *   mbr_order_dev int32 [B][K]: the ranks by ascending risk under the same tie rule; the ranks that are not real come
 *            last, in their original order.
 * With SCTC_MBR_CONF: utterance b owns the slots from sum_{q<b} max_{k<K_b[q]} n_{q,k} of conf_dev (double), n the
 * host's bound on the unit count: U_b in character unit, ceil(U_b / 2) in word unit.  For every real j the chosen
 * hypothesis (a) is aligned with hypothesis j (b) by the path of sctc_edit_distance_batch (the first of MATCH / UP /
 * LEFT / SUB, the leftover rule); match_j[i] = 1 where the path has MATCH at unit i of a, and match_best[i] = 1.
 *   conf[i] = (sum_j w_j * match_j[i], ascending j over the real ranks) / Z;  conf_len_dev int32 [B]: the unit count
 * of the chosen hypothesis, 0 without one.  Slots past conf_len are not written.  The chosen index is read on the
 * device.  Without the flag both pointers are NULL.
 * SCTC_ERR_ARG (no device needed): NULL config, arrays or outputs, B < 0, K outside 1..256, unknown unit or flags,
 * K_b outside [0, K], a length outside 0..4095, a negative offset, A outside 1..256, space outside [1, A) in word
 * unit, a scale that is not finite or is < 0; SCTC_ERR_WORKSPACE: workspace too small.  B == 0 launches nothing.
 * Apart from the interning's table (see there) no atomics; deterministic bit for bit.  Allocates no device memory;
 * the descriptors go through the calling thread's pinned host buffer into the workspace: a call waits for the
 * previous call of the same thread to have read its descriptors, so it cannot be recorded into a stream capture
 * (hipGraph), as sctc_edit_distance_batch. */
int sctc_nbest_mbr_batch(const sctc_mbr_config* cfg, const int32_t* labels_dev, const double* scores_dev,
                         const int32_t* order_dev, double* post_dev, double* risk_dev, int32_t* best_dev,
                         int32_t* mbr_order_dev, int32_t* dist_dev, double* conf_dev, int32_t* conf_len_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- CTC loss on a time-major [T, N, C] tensor: what torch.nn.functional.ctc_loss takes (ctc_torch.py) -----
 * Added without an ABI version bump (still 6): sctc_ctc_tnc_probs, sctc_ctc_tnc_empty, sctc_ctc_tnc_grad
 * (DESIGN.md §4.13).
 *
 * A contiguous [T * N][C] buffer is a batch of sctc_ctc_loss_batch as it stands: frame t of utterance n is row
 * rowbase_dev[t] + frame_off[n] with rowbase[t] = t * N, frame_off[n] = n, ld = C.  The three entries are what
 * surrounds that call: the prologue that fills the buffer from a tensor of any strides, the utterances with an empty
 * target (U == 0, which sctc_ctc_loss_batch rejects and torch.nn.functional.ctc_loss allows), and the backward pass
 * of the autograd function.  T_n_dev (device int32 [N], 1..T) holds the frames of every utterance: rows of the padded
 * frames t >= T_n[n] are never read, and written only by sctc_ctc_tnc_grad (zeros).  None of the kernels uses atomics
 * or waits for another workgroup: each is deterministic bit for bit. */

#define SCTC_TNC_LOG_PROBS 0  /* the input holds log-probabilities (torch.nn.functional.ctc_loss): p = exp(x) */
#define SCTC_TNC_LOGITS 1     /* unnormalised activations: p = softmax of the row, the arithmetic of sctc_softmax_rows */

typedef struct sctc_tnc_config {
    int32_t T, N, C;              /* frames, utterances (>= 0), alphabet incl. the blank (>= 1); T * N <= INT32_MAX */
    int32_t dtype;                /* SCTC_F32 | SCTC_F64: type of the strided tensor, of probs and of the gradient rows */
    int32_t mode;                 /* SCTC_TNC_LOG_PROBS | SCTC_TNC_LOGITS */
    int32_t blank;                /* blank id, 0..C-1 (torch.nn.CTCLoss(blank=)) */
    int64_t stride_t, stride_n, stride_c;   /* element strides of the strided [T, N, C] tensor: the input of
                                               sctc_ctc_tnc_probs, the output of sctc_ctc_tnc_grad */
} sctc_tnc_config;

/* All three: SCTC_ERR_ARG (no device needed) for a NULL config, T < 0, N < 0, C < 1, a blank outside [0, C), an
 * unknown dtype or mode, T * N beyond INT32_MAX (rowbase is int32), and a NULL pointer with work to do.  T == 0 or
 * N == 0 launches nothing.  No entry allocates device memory; every launch goes to `stream`. */

/* The prologue of ctc_torch.ctc_loss: probs_dev [T * N][C] (contiguous) from the strided input_dev, row t * N + n
 * for t < T_n[n].  A row per lane for C <= 32, a row per wave beyond. */
int sctc_ctc_tnc_probs(const sctc_tnc_config* cfg, const void* input_dev, const int32_t* T_n_dev, void* probs_dev,
                       void* stream);

/* Utterances with an empty target, one wave each: idx_dev (device int32 [n_idx], 0 <= n_idx <= N) lists them.
 * cost_dev[n] = -sum_t log p[t, n, blank], summed in float64 in ascending t; grad_dev rows p[t, n, :] - onehot(blank)
 * (layout of probs_dev); skip_dev[n] = 1 and cost +inf if a p[t, n, blank] is 0, else 0.  cost_dev double [N],
 * skip_dev int32 [N]: only the listed entries are written.  n_idx == 0 launches nothing.
 * sym_dev (device int32 [n_idx], 0..C-1, or NULL: the blank for all): the symbol that listed utterance i emits in
 * every frame, in place of the blank.  It serves the one other utterance with a single alignment, one label in one
 * frame (T_n == 1, U == 1): PyTorch's loss there is -log p[0, n, label], while ctc_fast.pyx:42-47 normalises frame 0
 * over the blank and the label before any band applies and returns -log(p_blank + p_label), and so does
 * sctc_ctc_loss_batch. */
int sctc_ctc_tnc_empty(const sctc_tnc_config* cfg, const void* probs_dev, const int32_t* T_n_dev, const int32_t* idx_dev,
                       const int32_t* sym_dev, int32_t n_idx, void* grad_dev, double* cost_dev, int32_t* skip_dev,
                       void* stream);

/* The backward pass of ctc_torch.ctc_loss: out[t, n, c] (strided) = scale_dev[n] * grad_dev[t * N + n][c] (one
 * float64 product, rounded once) where t < T_n[n], skip_dev[n] == 0 and cost_dev[n] is finite; exactly 0 elsewhere,
 * by select: the gradient rows of the other frames and utterances are not read (they may hold anything, NaN
 * included).  scale_dev double [N]. */
int sctc_ctc_tnc_grad(const sctc_tnc_config* cfg, const void* grad_dev, const int32_t* T_n_dev, const double* cost_dev,
                      const int32_t* skip_dev, const double* scale_dev, void* out_dev, void* stream);

/* ---- minimum word error rate training over n-best lists (ctc_torch.mwer_loss) -----
 * Added without an ABI version bump (still 6): sctc_ctc_mwer_probs, sctc_ctc_mwer_coef, sctc_ctc_mwer_combine.
 *
 * Utterance n of a time-major [T, N, C] tensor has frames T_n and hypotheses k < K_n[n] <= K with label rows y_k
 * (length U_k >= 0, labels in [0, C), none equal to the blank) and errors W_k (float64, any unit the caller likes).
 *   ll_k     = log P_ctc(y_k | x_n), float64: minus the cost the CTC kernels return for that label row over that
 *              utterance's probabilities.
 *   real     hypothesis k is REAL when k < K_n[n], W_k is finite, the CTC call's skip is 0 and its cost is finite.
 *            Everything else has weight 0 and is never read beyond that test.
 *   active   an utterance is ACTIVE when T_n >= 2 and it has at least one real hypothesis.  An inactive utterance has
 *            loss 0 and gradient rows of exact zeros.  (One frame is the shape where the CTC kernels follow the
 *            reference to -log(p_blank + p_label) instead of the CTC loss; MWER over one frame is of no use, so it is
 *            left out, not special-cased.)
 *   weights  m = max ll_k over the real ones; w_k = exp(scale * (ll_k - m)), exactly 1.0 where ll_k == m;
 *            Z = sum w_k in ascending k; P_k = w_k / Z; R = sum P_k * W_k in ascending k, the expected error;
 *            Wbar = (sum W_k, ascending k) / (number of real hypotheses).  All float64, no contraction.
 *   loss     loss_n = R - Wbar, or R alone with subtract_mean == 0.  The baseline changes the value, never the
 *            gradient.
 *   coef     c_k = scale * P_k * (W_k - R) = d loss_n / d ll_k.
 *   gradient d loss_n / d input[t, n, c] = sum_k c_k * occ_k[t, c] for t < T_n, exact 0 for padded frames, where
 *            occ_k = p - g_k is the occupancy of symbol c at frame t under hypothesis k, p the probabilities and g_k
 *            the gradient row the CTC kernels return.  Because sum_k c_k = 0 the p term cancels: the sum is the exact
 *            derivative both with respect to activations in front of a softmax and with respect to raw
 *            log-probabilities.
 *
 * The scheme: a buffer [T][N * K][C] is a batch of sctc_ctc_loss_batch as it stands, with rowbase[t] = t * N * K,
 * frame_off = n * K + k and ld = C, and a [T, N * K, C] batch of sctc_ctc_tnc_empty (the hypotheses with U == 0).  The
 * three entries are what surrounds those calls.  Each returns SCTC_ERR_ARG (no device needed) for a NULL config, T < 0,
 * N < 0, K outside 1..256, C < 1, an unknown dtype or mode, T * N * K beyond INT32_MAX, a scale that is not finite or
 * is < 0, a subtract_mean other than 0 and 1, and a NULL pointer with work to do.  T == 0 or N == 0 launches nothing.
 * No entry allocates device memory; every launch goes to `stream`; no float atomics and no waiting on another
 * workgroup: each is deterministic bit for bit. */
typedef struct sctc_mwer_config {
    int32_t T, N, K, C;           /* frames, utterances (>= 0), hypotheses per utterance (1..256), alphabet (>= 1) */
    int32_t dtype;                /* SCTC_F32 | SCTC_F64: type of the strided tensor, of probs, the gradient rows and G */
    int32_t mode;                 /* SCTC_TNC_LOG_PROBS | SCTC_TNC_LOGITS */
    int64_t stride_t, stride_n, stride_c;   /* element strides of the strided [T, N, C] input of sctc_ctc_mwer_probs */
    double scale;                 /* finite, >= 0: multiplies the log-likelihood differences */
    int32_t subtract_mean;        /* 0 | 1 */
} sctc_mwer_config;

/* The prologue, §4.13's (exp of log-probabilities, or the softmax in the arithmetic of sctc_softmax_rows), computed
 * once per (t, n) from the strided input_dev and stored to the K_n[n] consecutive rows (t * N + n) * K + k of
 * probs_dev [T * N * K][C].  T_n_dev, K_n_dev device int32 [N].  Padded frames t >= T_n[n] and ranks >= K_n[n] are
 * neither read nor written.  A row per lane for C <= 32, a row per wave beyond. */
int sctc_ctc_mwer_probs(const sctc_mwer_config* cfg, const void* input_dev, const int32_t* T_n_dev, const int32_t* K_n_dev,
                        void* probs_dev, void* stream);

/* One wave per utterance.  cost_dev double [N * K], skip_dev int32 [N * K]: what the CTC calls returned for pair
 * n * K + k (any finite or non-finite value where none was made: the caller marks those with skip != 0);
 * errors_dev double [N * K].  Outputs: loss_dev double [N]; coef_dev double [N * K], exact +0.0 where the rank is not
 * real or the utterance inactive; posterior_dev double [N * K], 0 there; expected_dev double [N], R (0 when inactive);
 * real_dev int32 [N * K], 1 for the real ranks of an active utterance; inactive_dev int32 [N]. */
int sctc_ctc_mwer_coef(const sctc_mwer_config* cfg, const double* cost_dev, const int32_t* skip_dev, const double* errors_dev,
                       const int32_t* T_n_dev, const int32_t* K_n_dev, double* loss_dev, double* coef_dev,
                       double* posterior_dev, double* expected_dev, int32_t* real_dev, int32_t* inactive_dev, void* stream);

/* out_dev [T * N][C] (contiguous): row t * N + n is sum over the real k, ascending, of coef_k * (double(p) -
 * double(g_k)), rounded once to dtype, for t < T_n[n] of the active utterances; the other rows are not written.
 * probs_dev, grad_dev [T * N * K][C]: the prologue's output and the gradient rows of the CTC calls.  By select: no row
 * of a rank that is not real is read; p is read from the first real rank's row (every rank's row of a (t, n) holds the same p).
 * The result is a gradient buffer of sctc_ctc_tnc_grad with skip = inactive and cost = 0. */
int sctc_ctc_mwer_combine(const sctc_mwer_config* cfg, const void* probs_dev, const void* grad_dev, const double* coef_dev,
                          const int32_t* real_dev, const int32_t* T_n_dev, const int32_t* inactive_dev, void* out_dev,
                          void* stream);

/* ---- BRNN: ctc_fast/nnets/brnnet.py NNet ------------------------------- */

typedef struct sctc_brnn_config {
    int32_t input_dim;       /* inputDim   brnnet.py:10 */
    int32_t output_dim;      /* outputDim  (alphabet incl. blank) */
    int32_t layer_size;      /* layerSize  */
    int32_t num_layers;      /* numLayers  */
    int32_t temporal_layer;  /* temporalLayer; <=0 or >=numLayers means none (brnnet.py:27-30) */
    int32_t max_frames;      /* capacity in frames summed over the minibatch (maxBatch for B=1) */
    int32_t max_utts;        /* capacity in utterances per call (1 = reference semantics) */
    float max_act;           /* maxAct = 20.0 (brnnet.py:32); <= 0 disables the ceiling (rnnetcpu.py) */
    float reg;               /* L2 coefficient (brnnet.py:22) */
    int32_t train;           /* 0: forward-only model (train=False) */
    int32_t operand_dtype;   /* SCTC_F32 (0, default): the reference's fp32 arithmetic everywhere.
                                SCTC_F16: the "fp16 activations" configuration (BASELINE configs[4]):
                                the operands of every time-batched contraction and of the
                                6..16-utterance recurrent step are rounded to 16 bit (float16 in
                                the forward pass, bfloat16 in the backward pass: deltas need
                                fp32's exponent range), products exact, accumulation fp32;
                                parameters, gradients, activations in memory, softmax and the
                                CTC lattices (float64) are unchanged.
                                SCTC_BF16X3: fp32 semantics everywhere (same tolerances as SCTC_F32);
                                only the time-batched contractions change instruction: each fp32
                                operand is split exactly into three bfloat16 terms and six cross
                                products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
                                (dropped terms <= 2^-23 of a product); recurrent step, softmax, CTC
                                and the update stay on the fp32 / fp64 paths */
} sctc_brnn_config;

/* One parameter tensor of `stack` (brnnet.py:58-59,71-72): order
 * [W1,b1] ... [W_{NL+1},b_{NL+1}] [Wf] [Wb]; stored row-major [rows][ld] inside the
 * flat parameter buffer (ld = rows/cols rounded up, zero padded). */
typedef struct sctc_tensor_info {
    int64_t offset;  /* element offset in the flat params / grads buffers */
    int32_t rows, cols, ld, kind; /* kind: 0 weight, 1 bias (cols == 1, ld == 1), 2 recurrent */
} sctc_tensor_info;

typedef struct sctc_brnn_sizes {
    int64_t param_elems;      /* floats in the flat (padded) parameter buffer */
    int64_t param_count;      /* unpadded count == NNet.paramCount() minus the dummy biases */
    size_t workspace_bytes;   /* device workspace for activations, deltas, CTC lattices */
    int32_t n_tensors;        /* 2*(NL+1) (+2 when there is a temporal layer) */
} sctc_brnn_sizes;

typedef struct sctc_brnn* sctc_brnn_t;

int sctc_brnn_query(const sctc_brnn_config* cfg, sctc_brnn_sizes* out);
/* NNet.__init__/initParams buffers (brnnet.py:10-86).  params/grads: device float[param_elems]
 * owned by the caller for the lifetime of the handle (grads may be NULL when !train). */
int sctc_brnn_create(const sctc_brnn_config* cfg, float* params_dev, float* grads_dev,
                     void* workspace_dev, size_t workspace_bytes, sctc_brnn_t* out);
int sctc_brnn_destroy(sctc_brnn_t h);
int sctc_brnn_tensor_info(sctc_brnn_t h, int32_t index, sctc_tensor_info* out);

/* Minibatch descriptor.  feats_dev: float [sum T][input_dim], utterances
 * concatenated in caller order, each one the reference's (inputDim,T) F-order array. */
typedef struct sctc_minibatch {
    int32_t B;
    const int32_t* T_b;       /* host [B] */
    const float* feats_dev;
    const int32_t* labels;    /* host concatenated (NULL for forward only) */
    const int32_t* U_b;       /* host [B] */
} sctc_minibatch;

#define SCTC_FLAG_SYNC_SKIP 1   /* reference B=1 semantics: look at `skip` on the host before
                                   the backward pass; if every utterance is skipped, return
                                   with the gradients untouched (brnnet.py:185-186) */
#define SCTC_FLAG_ACCUMULATE 2  /* add into grads instead of overwriting */
#define SCTC_FLAG_NO_REG_GRAD 4 /* leave the L2 term reg*W (brnnet.py:197-198,244-247) out of the
                                   gradients: minibatch / data-parallel callers add it ONCE, after
                                   the all-reduce and the 1/n_valid scaling (sctc_sumsq_reg,
                                   sctc_nesterov_step_reg) */

/* NNet.costAndGrad(data, labels) (brnnet.py:117-249) for a minibatch: forward,
 * softmax + CTC, backward.  Gradients are SUMMED over utterances (and frames) into
 * grads_dev; skipped utterances contribute zero.
 *   cost_host/skip_host [B] (optional, forces a stream sync), caller order;
 *   costs include nothing of the L2 term: *regcost_host (optional) receives
 *   sum (reg/2)*||w||^2 over all weight tensors (brnnet.py:178-183).                     */
int sctc_brnn_cost_and_grad(sctc_brnn_t h, const sctc_minibatch* mb, int32_t flags,
                            double* cost_host, int32_t* skip_host, double* regcost_host,
                            void* stream);
/* same, results stay on the device (no host sync): cost_dev double[B], skip_dev int32[B].
 * The caller must follow up with sctc_brnn_check before trusting the results. */
int sctc_brnn_cost_and_grad_async(sctc_brnn_t h, const sctc_minibatch* mb, int32_t flags,
                                  double* cost_dev, int32_t* skip_dev, void* stream);
/* Data-parallel overlap ("bucket by layer and launch as each wgrad GEMM finishes",
 * output layer first, brnnet.py:191-193): the hipEvent_t the engine records on the step's stream
 * right after the gradient of parameter tensor `index` is final (a weight tensor's event covers
 * its bias; NULL for bias indices), and hipStreamWaitEvent for a caller that only holds raw
 * stream pointers -- a side stream waits for tensor i's event and starts its all-reduce while
 * the backward pass continues.  The weight gradients of the layers above the temporal layer
 * are final before the BPTT recurrence starts; their events are recorded only after it has retired, so that no
 * collective kernel occupies compute units while the persistent BPTT grid (which needs all of
 * its workgroups resident at once) is being placed. */
void* sctc_brnn_grad_event(sctc_brnn_t h, int32_t index);
int sctc_stream_wait_event(void* stream, void* event);
/* SURVEY 8(e) (the reference has no multi-GPU path): the ONE exchange step of the data-parallel path as a C entry --
 * the sum of the weight gradients over the ranks of an RCCL communicator, overlapped with the backward pass that
 * sctc_brnn_cost_and_grad_async queued on `compute_stream`.  `side_stream` (a stream of its own) waits for the
 * event of each layer's gradient in the order the backward pass finishes them (output layer first; the layers above
 * the temporal layer and the recurrent pair after BPTT has retired) and starts ncclAllReduce(sum, float, in place)
 * on that layer's slice of the flat gradient buffer; `side_dev` (nullable: double[side_count] on the device, e.g.
 * [n_valid, cost_sum, regcost, has_regcost], produced on the compute stream) is reduced last; on return
 * `compute_stream` has been made to wait for all of it (nothing is synchronised with the host).
 *   rccl_comm        an ncclComm_t the caller created for this rank's device (ncclCommInitRank), one per rank
 *   backward_queued  0: this rank queued no backward pass this step (empty shard, gradient buffer zeroed on the
 *                    compute stream): the side stream is ordered behind the compute stream as a whole
 * librccl.so is resolved with dlopen at first use (libsctc_hip.so does not link against it): SCTC_ERR_STATE if it is
 * not there.  The Python host side (dist_sgd.allreduce_overlapped) issues the same sequence through
 * torch.distributed; this entry is for hosts that own their communicator. */
int sctc_brnn_allreduce_grads(sctc_brnn_t h, void* rccl_comm, void* compute_stream, void* side_stream,
                              double* side_dev, int32_t side_count, int32_t backward_queued);
/* synchronises `stream` and reports a failure of the asynchronous work queued on it:
 * SCTC_ERR_TIMEOUT when a persistent recurrent kernel gave up waiting for its peers (results of
 * that call are then meaningless), SCTC_OK otherwise */
int sctc_brnn_check(sctc_brnn_t h, void* stream);
/* which recurrence the last step ran (diagnostics / tests): 1 = one persistent launch per pass,
 * 2 = the same under the device lease, 3 = the non-persistent fallback (one launch per time step;
 * taken when a persistent grid cannot be co-resident: layer sizes beyond 2048 units, CU masks, a
 * step re-run after SCTC_ERR_TIMEOUT, SCTC_REC_VARIANT=3), 0 = none yet; *retries = steps of this
 * handle that were re-run after a timeout.  Any pointer may be NULL. */
int sctc_brnn_recurrent_path(sctc_brnn_t h, int32_t* forward_path, int32_t* bptt_path, int32_t* retries);
/* the order the last backward pass of the handle ran in (read-only; diagnostics / tests): 0 = serial, 1 = the weight
 * gradients above the temporal layer beside the default BPTT grid, 2 = beside the half-grid BPTT (SCTC_BWD_OVERLAP,
 * INTEGRATION.md); negative: null handle */
int sctc_brnn_bwd_overlap_mode(sctc_brnn_t h);

/* NNet(train=False).costAndGrad(data) (brnnet.py:171-173): probs_dev float [sum T][output_dim],
 * caller order, each utterance the reference's (outputDim,T) F-order probs */
int sctc_brnn_forward(sctc_brnn_t h, const sctc_minibatch* mb, float* probs_dev, void* stream);

/* The CTC scratch of a step lives in the model's workspace, which reserves 2048 lattice states (2U+1) per frame and
 * utterance slot.  The reference bounds no label row (ctc_fast.pyx:22-32 allocates (2U+1) x T per call): a minibatch
 * with a longer row may need more.  sctc_brnn_ctc_workspace_bytes says how much THIS minibatch needs (*needed) and
 * how much the handle currently offers (*reserved: its own share, or what was last set); a caller that finds
 * needed > reserved allocates a device buffer of at least `needed` bytes and hands it over with
 * sctc_brnn_set_ctc_workspace -- it replaces the built-in share for all later steps and stays OWNED BY THE CALLER, who
 * keeps it alive until it sets another one, resets (dev = NULL) or destroys the handle.  Without this a step whose
 * CTC scratch does not fit returns SCTC_ERR_WORKSPACE.  (nnets/brnnet.py does this by itself: round 6.) */
int sctc_brnn_ctc_workspace_bytes(sctc_brnn_t h, const sctc_minibatch* mb, size_t* needed, size_t* reserved);
int sctc_brnn_set_ctc_workspace(sctc_brnn_t h, void* workspace_dev, size_t workspace_bytes);

/* ---- MWER inside the step: the BRNN trained on expected word error -----
 * Added without an ABI version bump (still 6): sctc_brnn_mwer_cost_and_grad, sctc_brnn_mwer_cost_and_grad_async,
 * sctc_brnn_mwer_workspace_bytes, sctc_brnn_set_mwer_workspace.
 *
 * One forward pass, the CTC recursions of every hypothesis (and of the reference), one backward pass.  Utterance b
 * (caller order) of the minibatch has frames T_b and hypotheses k < K_b[b] <= K with label rows y_{b,k} (length U >= 0,
 * labels in [1, A): the blank, 0, is an argument error) and errors W_{b,k} (float64).  real, active, weights, loss,
 * coefficients and the gradient with respect to the output layer's activations are those of the MWER block above
 * (n = b; the baseline is subtract_mean).  Three additions:
 *   ctc_weight   lambda, finite and >= 0.  With lambda > 0 the reference rows mb->labels / mb->U_b are required (U >= 1,
 *                as in sctc_brnn_cost_and_grad); the step's loss is loss_b + lambda * ctc_b and the output-layer gradient
 *                sum_k c_k (p - g_k) + lambda * g_ref.  An utterance whose reference CTC call skips, or whose cost is not
 *                finite, contributes no lambda term.  The reference row is never part of the posterior.  With lambda == 0
 *                the reference labels are not read and may be NULL; ctc_cost and ctc_skip then come back 0.
 *   empty        a hypothesis with U == 0 (all blank) is real: cost -sum_t log p[t, blank] in ascending t, gradient rows
 *                p - onehot(blank); skip and cost +inf when a p_blank is 0.
 *   inactive     an utterance with T_b < 2 or without a real hypothesis leaves exact zeros in its rows of the output
 *                layer's delta; with lambda > 0 and a usable reference row it gets lambda * g_ref.
 * hyp_U and errors are host [B * K], b-major; hyp_labels is concatenated over the slots the contract reads, in that
 * order: a slot with k >= K_b[b] or a non-finite error carries no labels, and neither its labels nor its hyp_U are
 * looked at.  Gradients are summed over utterances like sctc_brnn_cost_and_grad's, under the same SCTC_FLAG_ACCUMULATE
 * and SCTC_FLAG_NO_REG_GRAD; SCTC_FLAG_SYNC_SKIP is SCTC_ERR_ARG here.  Two runs are bit-equal: no float atomics, no
 * waiting on another workgroup in the kernels this adds. */
typedef struct sctc_mwer_minibatch {
    int32_t K;                  /* hypothesis slots per utterance, 1..256 */
    const int32_t* K_b;         /* host [B], 0..K */
    const int32_t* hyp_labels;  /* host, concatenated (may be NULL when no slot that is read has a label) */
    const int32_t* hyp_U;       /* host [B * K] */
    const double* errors;       /* host [B * K] */
    double scale;               /* finite, >= 0 */
    int32_t subtract_mean;      /* 0 | 1 */
    double ctc_weight;          /* finite, >= 0 */
} sctc_mwer_minibatch;

/* every pointer optional (a NULL struct: no outputs); caller order; host pointers for sctc_brnn_mwer_cost_and_grad,
 * device pointers for the _async entry */
typedef struct sctc_mwer_outputs {
    double* loss;       /* [B]  loss_b + lambda * ctc_b */
    double* expected;   /* [B]  R, the expected error (0 when inactive) */
    int32_t* inactive;  /* [B] */
    double* ctc_cost;   /* [B]  the reference row's CTC cost (lambda > 0) */
    int32_t* ctc_skip;  /* [B]  1 where that call skipped or its cost is not finite: no lambda term */
    double* posterior;  /* [B * K]  P_k, 0 where not real */
    int32_t* real;      /* [B * K] */
} sctc_mwer_outputs;

/* The step's device workspace is owned by the caller (the sctc_brnn_set_ctc_workspace pattern): the two K-fold buffers
 * [N * S][A] float (S = K, + 1 with lambda > 0), the CTC workspace of the label rows and the small per-slot arrays
 * (csrc/brnn_mwer_plan.h).  sctc_brnn_mwer_workspace_bytes validates the minibatch and the descriptor exactly as the
 * step does and says how much THIS minibatch needs; sctc_brnn_set_mwer_workspace hands a 256-byte aligned buffer over
 * (NULL and 0: none), which the caller keeps alive until it sets another one or destroys the handle.  A step without
 * enough workspace returns SCTC_ERR_WORKSPACE.  sctc_brnn_query's answer does not include it. */
int sctc_brnn_mwer_workspace_bytes(sctc_brnn_t h, const sctc_minibatch* mb, const sctc_mwer_minibatch* mw, size_t* needed);
int sctc_brnn_set_mwer_workspace(sctc_brnn_t h, void* workspace_dev, size_t workspace_bytes);

/* SCTC_ERR_ARG before any launch: a NULL handle, minibatch, descriptor or descriptor field, K outside 1..256, a K_b
 * outside 0..K, a negative hyp_U or a label outside [1, A) in a slot that is read, a scale or ctc_weight that is not
 * finite or is < 0, a subtract_mean other than 0 and 1, N * S beyond INT32_MAX, SCTC_FLAG_SYNC_SKIP, a model created
 * with train = 0.  The scalars of the descriptor are checked first, without a device or a handle.
 * The step is re-run after SCTC_ERR_TIMEOUT like sctc_brnn_cost_and_grad's (not when accumulating); its CTC and MWER
 * kernels are timed under SCTC_PHASE_CTC.  *regcost_host as in sctc_brnn_cost_and_grad. */
int sctc_brnn_mwer_cost_and_grad(sctc_brnn_t h, const sctc_minibatch* mb, const sctc_mwer_minibatch* mw, int32_t flags,
                                 const sctc_mwer_outputs* out_host, double* regcost_host, void* stream);
/* same, the outputs stay on the device (no host sync); follow up with sctc_brnn_check */
int sctc_brnn_mwer_cost_and_grad_async(sctc_brnn_t h, const sctc_minibatch* mb, const sctc_mwer_minibatch* mw, int32_t flags,
                                       const sctc_mwer_outputs* out_dev, void* stream);

/* rocprof-free timing hooks: milliseconds spent in the phases of the last call, measured with hipEvents
 * on the step's stream.  sctc_brnn_set_profiling(h, 1): exact phase timers that synchronise the
 * stream at every phase change (perturbing); (h, 2): asynchronous -- one event per phase change is
 * recorded and only resolved by sctc_brnn_phase_ms after the step, no host sync is added, so it can
 * stay on while a benchmark times its steps (bench.py's roofline leg); (h, 0): off */
#define SCTC_PHASE_FWD_GEMM 0
#define SCTC_PHASE_FWD_REC 1
#define SCTC_PHASE_CTC 2
#define SCTC_PHASE_BWD_GEMM 3
#define SCTC_PHASE_BWD_REC 4
#define SCTC_PHASE_OTHER 5
#define SCTC_N_PHASES 6
int sctc_brnn_set_profiling(sctc_brnn_t h, int32_t enable);
/* diagnostics only: device pointer / shape of an internal fp32 matrix of the last call (which:
 * 0..numLayers = hActs[i] (0 = the packed input), 100 / 101 = hActsFor / hActsBack, 102 = the temporal
 * layer's W h + b, 200 = the delta entering layer 1, 201 / 202 = deltasFor / deltasBack as the BPTT
 * recurrence left them); rows follow the packed time-major layout (one utterance: row t = frame t).
 * Lets a test separate the error of one contraction from the error of its operands.  With
 * operand_dtype = SCTC_F16 the hidden ReLU layers (1..numLayers) and 200 have no fp32 copy: see below. */
int sctc_brnn_debug_buffer(sctc_brnn_t h, int32_t which, void** dev_ptr, int64_t* rows, int64_t* cols,
                           int64_t* ld);
/* diagnostics only, operand_dtype = SCTC_F16: the 16-bit shadows the GEMMs read, as raw uint16 in the same
 * layout; *dtype says how to read them.  SCTC_F16: which = 0..numLayers, the forward operands hActs[i].
 * SCTC_BF16 (training models, after a cost_and_grad call): 50..50+numLayers = the weight gradients' copies
 * of hActs[i], 100 / 101 = hActsFor / hActsBack, 200 = the delta entering layer 1, 201 / 202 = deltasFor /
 * deltasBack, 203 = what the other of the two alternating delta buffers was left with (the delta entering
 * layer 2). */
int sctc_brnn_debug_buffer16(sctc_brnn_t h, int32_t which, void** dev_ptr, int64_t* rows, int64_t* cols,
                             int64_t* ld, int32_t* dtype);
/* diagnostics only: per-step s_memtime stamps of the recurrent kernel when SCTC_REC_DEBUG=1 */
int sctc_brnn_debug_read(sctc_brnn_t h, uint32_t* out, int32_t n_words);
int sctc_brnn_phase_ms(sctc_brnn_t h, float* ms_out /* [SCTC_N_PHASES] */);
/* algorithmic FLOPs of one cost_and_grad over this minibatch, SURVEY 8(d) formula
 * (total, and the part in the time-batched GEMMs / in the recurrent steps) */
int sctc_brnn_flops(sctc_brnn_t h, const sctc_minibatch* mb, double* total, double* gemm,
                    double* recurrent);

/* cm.dot(A, B, target=C) of cudamat on row-major fp32 device matrices (brnnet.py:140 forward,
 * :196 weight gradient, :204 delta propagation, :227-230 recurrent weight gradient):
 *   C[M][N] = sum_k A(m,k) B(k,n) (+ bias[n]) (relu)
 *   a_kcontig: A(m,k) = A[m*lda+k], else A[k*lda+m];  b_kcontig: B(k,n) = B[n*ldb+k], else B[k*ldb+n]
 * fp32 operands, fp32 accumulate on the matrix cores (v_mfma_f32_32x32x2_f32).
 * workspace (optional) enables deterministic split-K for small M*N. */
int sctc_gemm_f32(const float* A_dev, int64_t lda, int32_t a_kcontig, const float* B_dev,
                  int64_t ldb, int32_t b_kcontig, float* C_dev, int64_t ldc, int32_t M, int32_t N,
                  int32_t K, const float* bias_dev, int32_t relu, void* workspace_dev,
                  size_t workspace_bytes, void* stream);

/* The same contraction with both operands ROUNDED to a 16-bit type (operand_dtype = SCTC_F16 or
 * SCTC_BF16, round-to-nearest-even) on their way to the matrix cores and fp32 accumulation
 * (v_mfma_f32_32x32x16_f16 / _bf16): the GEMM of the "fp16 activations" configuration
 * (BASELINE configs[4]).  Operands and result stay fp32 in memory.
 * operand_dtype = SCTC_BF16X3: no rounding -- the three-term split described at sctc_brnn_config.
 * operand_dtype | SCTC_OPERANDS_16BIT (SCTC_F16 / SCTC_BF16 only): the operands are 16-bit in memory already
 * (both in the SAME layout: a_kcontig == b_kcontig, lda / ldb multiples of 8 elements); large problems
 * then run on the LDS-DMA staged kernel (csrc/gemm_g16.hip), the path the engine's GEMMs take. */
int sctc_gemm_h16(const float* A_dev, int64_t lda, int32_t a_kcontig, const float* B_dev,
                  int64_t ldb, int32_t b_kcontig, float* C_dev, int64_t ldc, int32_t M, int32_t N,
                  int32_t K, const float* bias_dev, int32_t relu, int32_t operand_dtype,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- what sgd.py needs from cudamat objects (sgd.py:21-23,93-106,129-141,161) ---- */

/* y += alpha * x   (CUDAMatrix.add_mult, NNet.updateParams brnnet.py:251-256) */
int sctc_axpy(float* y_dev, const float* x_dev, float alpha, int64_t n, void* stream);
/* x *= alpha       (CUDAMatrix.mult) */
int sctc_scale(float* x_dev, float alpha, int64_t n, void* stream);
/* sum of squares of n floats into *out_dev (double); euclid_norm()**2 over the whole
 * gradient stack in one launch instead of 14 host syncs (sgd.py:103-107) */
int sctc_sumsq(const float* x_dev, int64_t n, double* out_dev, void* workspace_dev,
               size_t workspace_bytes, void* stream);
/* Fused Nesterov step of sgd.py:129-141,161 on the flat buffers:
 *   alph = alpha * min(1, maxGNorm/gnorm)  with gnorm = sqrt(*sumsq_dev) * grad_scale
 *   v = mom*v - alph*grad_scale*g ;  w += v                                             */
int sctc_nesterov_step(float* w_dev, float* v_dev, const float* g_dev, int64_t n, float mom,
                       float alpha, float max_gnorm, float grad_scale, const double* sumsq_dev,
                       void* stream);

/* Minibatch / data-parallel form of the two calls above with the L2 term applied exactly once:
 * the effective gradient is  e = grad_scale * g + reg * (w + mom * v)  (g = SUM of the data
 * gradients over the minibatch, all-reduced over the ranks; grad_scale = 1/n_valid;
 * brnnet.py:197-198 adds reg*W to each utterance's gradient AT THE LOOK-AHEAD POINT w + mom*v
 * where sgd.py:91-95 evaluates it; w here is the weight after the look-ahead was undone
 * (sgd.py:97-100), v the velocity before this step's update; v_dev NULL = plain reg*w).
 *   sctc_sumsq_reg:          *out_dev = sum e^2 (float64 accumulation, two deterministic stages)
 *   sctc_nesterov_step_reg:  alph = alpha * min(1, maxGNorm / sqrt(*sumsq_dev));
 *                            v = mom*v - alph*e ;  w += v                                   */
/*   noreg_ranges_host: n_ranges (<= 128) ascending, disjoint element ranges [beg, end) of the flat
 *                      buffers that carry NO L2 term -- the biases (brnnet.py:197-200 regularises w only) */
int sctc_sumsq_reg(const float* g_dev, const float* w_dev, const float* v_dev, float mom,
                   float grad_scale, float reg, int64_t n,
                   const int64_t* noreg_ranges_host, int32_t n_ranges, double* out_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);
int sctc_nesterov_step_reg(float* w_dev, float* v_dev, const float* g_dev, int64_t n, float mom,
                           float alpha, float max_gnorm, float grad_scale, float reg,
                           const int64_t* noreg_ranges_host, int32_t n_ranges,
                           const double* sumsq_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCTC_H_ */
