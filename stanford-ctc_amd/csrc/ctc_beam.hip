// CTC prefix beam search on the device, the four of them: the n-gram
// search (beam_ngram.h), one search body (beam_search.h) instantiated with one LM policy (beam_policies.h)
// for each of the other three, and the host
// side of the four -- one plan of the workspace, one launch path, and per entry point only its own
// argument checks, its policy's arguments and its kernel.
#include <stdlib.h>

#include <vector>

#include "beam_lm.h"
#include "beam_ngram.h"
#include "beam_policies.h"

namespace sctc {
namespace {

using namespace beam;

__global__ __launch_bounds__(NT) void ctc_beam_kernel(NgramBeamArgs p) { ngram_beam_search(p); }

__global__ __launch_bounds__(NT) void ctc_lexbeam_kernel(BeamArgs p, LexiconArgs lx) { beam_search<LexiconPolicy>(p, lx); }

__global__ __launch_bounds__(NT) void ctc_lexngbeam_kernel(BeamArgs p, LexiconNgramArgs lx)
{
    beam_search<LexiconNgramPolicy>(p, lx);
}

__global__ __launch_bounds__(NT) void ctc_nnbeam_kernel(BeamArgs p, NNArgs nn) { beam_search<NNPolicy>(p, nn); }

__global__ __launch_bounds__(NT) void ctc_rnnbeam_kernel(BeamArgs p, RNNArgs nn) { beam_search<RNNPolicy>(p, nn); }

// the fields the four public config structs share, in their order; the sixth slot (`reserved`, or the
// lexicon search's `space`) is no concern of the plan or the launch
struct BeamView {
    int32_t B, A, dtype, beam, nbest;
    int64_t ld;
    const int32_t* T_b;
    const int64_t* frame_off;
    double alpha, beta;
};

template <typename Config>
BeamView view_of(const Config& c)
{
    return BeamView{c.B, c.A, c.dtype, c.beam, c.nbest, c.ld, c.T_b, c.frame_off, c.alpha, c.beta};
}

struct BeamPlan {
    std::vector<UttDesc> utt;
    size_t head = 0;     // descriptors + symbol map
    size_t total = 0;
};

// lm_rows: the search keeps LM rows for both beams; extra: further bytes per utterance of its policy
// (windows or states, one LM tile); what: the prefix of the entry point in the messages
int plan_beam(const BeamView& v, BeamPlan& pl, bool lm_rows, size_t extra, const char* what)
{
    SCTC_CHECK_ARG(v.B >= 1, "%s: empty batch", what);
    SCTC_CHECK_ARG(v.A >= 2 && v.A <= AMAX, "%s: alphabet size %d outside 2..%d", what, v.A, AMAX);
    SCTC_CHECK_ARG(v.beam >= 1 && v.beam <= KMAX, "%s: beam width %d outside 1..%d", what, v.beam, KMAX);
    SCTC_CHECK_ARG(v.nbest >= 1 && v.nbest <= v.beam, "%s: nbest %d outside 1..beam", what, v.nbest);
    SCTC_CHECK_ARG(v.dtype == SCTC_F32 || v.dtype == SCTC_F64, "%s: bad dtype %d", what, v.dtype);
    SCTC_CHECK_ARG(v.ld >= v.A, "%s: ld %lld < A %d", what, (long long)v.ld, v.A);
    SCTC_CHECK_ARG(v.T_b && v.frame_off, "%s: null T_b / frame_off", what);
    SCTC_CHECK_ARG(isfinite(v.alpha) && isfinite(v.beta), "%s: alpha / beta not finite", what);
    const int64_t M = (int64_t)v.beam * v.A;
    const size_t fixed = align256(2 * M * sizeof(float2)) + align256(M * sizeof(uint64_t)) +
                         (lm_rows ? align256(2 * M * sizeof(float)) : 0) + extra;
    pl.utt.resize(v.B);
    pl.head = align256(v.B * sizeof(UttDesc)) + align256(AMAX * sizeof(int32_t));
    size_t off = pl.head;
    int64_t id_off = 0;
    for (int b = 0; b < v.B; ++b) {
        const int T = v.T_b[b];
        SCTC_CHECK_ARG(T >= 0, "%s: utterance %d has %d frames", what, b, T);
        SCTC_CHECK_ARG(v.frame_off[b] >= 0, "%s: utterance %d has a negative frame offset", what, b);
        UttDesc& d = pl.utt[b];
        d.frame_off = v.frame_off[b];
        d.ws_off = (int64_t)off;
        d.id_off = id_off;
        d.T = T;
        d.pad = 0;
        off += fixed + align256((size_t)T * v.beam * sizeof(int32_t));
        id_off += T;
    }
    pl.total = off;
    return SCTC_OK;
}

// the symbol -> LM id map of a neural search; after plan_beam, which has checked A
int check_lm_ids(const int32_t* sym_word, int A, int V, const char* what)
{
    for (int c = 1; c < A; ++c)
        SCTC_CHECK_ARG(sym_word[c] >= 0 && sym_word[c] < V, "%s: symbol %d maps to LM id %d outside 0..%d", what, c,
                       sym_word[c], V - 1);
    return SCTC_OK;
}

int plan_ngram(const sctc_beam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "beam: null config");
    SCTC_TRY(plan_beam(view_of(*cfg), pl, cfg->lm != nullptr, 0, "beam"));
    if (cfg->lm) {
        SCTC_CHECK_ARG(cfg->sym_word, "beam: an LM needs the symbol -> word map");
        for (int c = 1; c < cfg->A; ++c)
            SCTC_CHECK_ARG(cfg->sym_word[c] >= 1 && cfg->sym_word[c] <= 255,
                           "beam: symbol %d maps to LM word %d outside 1..255", c, cfg->sym_word[c]);
    }
    return SCTC_OK;
}

// the lexicon search plans like the character search without an LM: the same workspace
int plan_lexicon(const sctc_lexbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "lexbeam: null config");
    SCTC_CHECK_ARG(cfg->lexicon, "lexbeam: null lexicon");
    SCTC_CHECK_ARG(cfg->A == cfg->lexicon->A, "lexbeam: alphabet size %d, the lexicon was built for %d", cfg->A,
                   cfg->lexicon->A);
    SCTC_CHECK_ARG(cfg->space >= 1 && cfg->space < cfg->A, "lexbeam: space symbol %d outside 1..A-1", cfg->space);
    return plan_beam(view_of(*cfg), pl, false, 0, "lexbeam");
}

// the neural LM search plans like the character search with an LM, plus its windows and LM tile
int plan_nn(const sctc_nnbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "nnbeam: null config");
    SCTC_CHECK_ARG(cfg->lm, "nnbeam: null LM");
    SCTC_CHECK_ARG(cfg->sym_word, "nnbeam: null symbol -> LM id map");
    const NNLMDev& m = cfg->lm->dev;
    SCTC_TRY(plan_beam(view_of(*cfg), pl, true, align256((size_t)2 * cfg->beam * WIN) + nn_tile_bytes(m.hmax, m.Vp, m.K),
                       "nnbeam"));
    return check_lm_ids(cfg->sym_word, cfg->A, m.V, "nnbeam");
}

// the recurrent LM search plans like the character search with an LM, plus the states of both beams
// and its LM tile
int plan_rnn(const sctc_rnnbeam_config* cfg, BeamPlan& pl)
{
    SCTC_CHECK_ARG(cfg, "rnnbeam: null config");
    SCTC_CHECK_ARG(cfg->lm, "rnnbeam: null LM");
    SCTC_CHECK_ARG(cfg->sym_word, "rnnbeam: null symbol -> LM id map");
    const RNNLMDev& m = cfg->lm->dev;
    SCTC_TRY(plan_beam(view_of(*cfg), pl, true,
                       align256((size_t)2 * cfg->beam * m.H * sizeof(float)) + rnn_tile_bytes(m.H, m.Vp), "rnnbeam"));
    return check_lm_ids(cfg->sym_word, cfg->A, m.V, "rnnbeam");
}

// the device side of a decode call as every entry point receives it
struct BeamIO {
    const void* probs;
    int32_t* ids;
    int32_t* lens;
    double* scores;
    void* ws;
    size_t ws_bytes;
    void* stream;
};

// The launch path of the four searches: the checks of the device arguments, the head of the workspace
// (descriptors, then the symbol map when the search has one: sym_word, nullptr for none; blank0 sets
// the blank's slot to 0), the common kernel arguments, and `launch(stream, args)`, which is the entry
// point's own hipLaunchKernelGGL.
// lm_device: the device the LM handle lives on, checked against the current one, or -1 for "not
// checked".  Only the recurrent search checks.  The other three handles record their device as well,
// but checking them would reject calls that work today across devices with peer access: a change of
// behaviour that wants a pull request of its own.
template <typename Launch>
int launch_beam(const char* what, const BeamView& v, const BeamPlan& pl, const BeamIO& io, const int32_t* sym_word,
                bool blank0, int lm_device, Launch&& launch)
{
    SCTC_CHECK_ARG(io.probs && io.lens && io.scores && io.ws, "%s: null device pointer", what);
    int64_t total_T = 0;
    for (int b = 0; b < v.B; ++b) total_T += v.T_b[b];
    SCTC_CHECK_ARG(io.ids || total_T == 0, "%s: null ids", what);
    if (io.ws_bytes < pl.total)
        return set_error(SCTC_ERR_WORKSPACE, "%s: workspace %zu bytes < %zu needed", what, io.ws_bytes, pl.total);
    if (lm_device >= 0) {
        int dev = 0;
        SCTC_HIP_TRY(hipGetDevice(&dev));
        SCTC_CHECK_ARG(dev == lm_device, "%s: the LM lives on device %d, the current device is %d", what, lm_device, dev);
    }
    hipStream_t s = (hipStream_t)io.stream;
    std::vector<char> head(pl.head, 0);
    memcpy(head.data(), pl.utt.data(), v.B * sizeof(UttDesc));
    const size_t sym_off = align256(v.B * sizeof(UttDesc));
    if (sym_word) {
        memcpy(head.data() + sym_off, sym_word, v.A * sizeof(int32_t));
        if (blank0) ((int32_t*)(head.data() + sym_off))[0] = 0;        // the blank has no LM id; never read
    }
    // small and synchronous with respect to the host buffer: a plain copy, then the launch
    SCTC_HIP_TRY(hipMemcpyAsync(io.ws, head.data(), pl.head, hipMemcpyHostToDevice, s));
    SCTC_HIP_TRY(hipStreamSynchronize(s));

    BeamArgs a{};
    a.probs = io.probs;
    a.ld = v.ld;
    a.f64 = v.dtype == SCTC_F64;
    a.A = v.A;
    a.K = v.beam;
    a.nbest = v.nbest;
    a.alpha = v.alpha;
    a.beta = v.beta;
    a.utt = (const UttDesc*)io.ws;
    a.sym_word = (const int32_t*)((char*)io.ws + sym_off);
    a.ws = (char*)io.ws;
    a.ids = io.ids;
    a.lens = io.lens;
    a.scores = io.scores;
    launch(s, a);
    SCTC_HIP_TRY(hipGetLastError());
    return SCTC_OK;
}

}  // namespace
}  // namespace sctc

using namespace sctc;

extern "C" {

size_t sctc_ctc_beam_workspace_bytes(const sctc_beam_config* cfg)
{
    BeamPlan pl;
    if (plan_ngram(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_beam_decode_batch(const sctc_beam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                               int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                               size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_ngram(cfg, pl));
    const sctc_lm* lm = cfg->lm;
    return launch_beam("beam", view_of(*cfg), pl,
                       BeamIO{probs_dev, ids_dev, lengths_dev, scores_dev, workspace_dev, workspace_bytes, stream},
                       lm ? cfg->sym_word : nullptr, false, -1, [&](hipStream_t s, const BeamArgs& a) {
                           NgramBeamArgs n{a.probs, a.ld, a.f64, a.A, a.K, a.nbest, a.alpha, a.beta, a.utt, a.sym_word, a.ws};
                           if (lm) {
                               n.lm_key = lm->key;
                               n.lm_prob = lm->prob;
                               n.lm_bo = lm->bo;
                               n.lm_mask = (uint64_t)(lm->cap - 1);
                               n.lm_order = lm->order;
                               n.lm_bos = lm->bos;
                           }
                           n.ids = a.ids;
                           n.lens = a.lens;
                           n.scores = a.scores;
                           hipLaunchKernelGGL(ctc_beam_kernel, dim3(cfg->B), dim3(NT), 0, s, n);
                       });
}

size_t sctc_ctc_lexbeam_workspace_bytes(const sctc_lexbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_lexicon(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_lexbeam_decode_batch(const sctc_lexbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_lexicon(cfg, pl));
    const sctc_lexicon* h = cfg->lexicon;
    const BeamIO io{probs_dev, ids_dev, lengths_dev, scores_dev, workspace_dev, workspace_bytes, stream};
    if (h->order) {   // a word n-gram LM: the kernel of its policy (§4.6b)
        LexiconNgramArgs ng{};
        ng.child = h->child;
        ng.word = h->word;
        ng.ug = h->ug;
        ng.bo = h->bo;
        ng.key = h->bg_key;
        ng.val = h->bg_val;
        ng.nbo = h->ng_bo;
        ng.id = h->ng_id;
        ng.mask = (uint64_t)(h->bg_cap - 1);
        ng.start = h->start;
        ng.space = cfg->space;
        ng.order = h->order;
        return launch_beam("lexbeam", view_of(*cfg), pl, io, nullptr, false, -1, [&](hipStream_t s, const BeamArgs& a) {
            hipLaunchKernelGGL(ctc_lexngbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, ng);
        });
    }
    LexiconArgs lx{};
    lx.child = h->child;
    lx.word = h->word;
    lx.ug = h->ug;
    lx.bo = h->bo;
    lx.key = h->bg_key;
    lx.val = h->bg_val;
    lx.mask = (uint64_t)(h->bg_cap - 1);
    lx.start = h->start;
    lx.space = cfg->space;
    return launch_beam("lexbeam", view_of(*cfg), pl, io,
                       nullptr, false, -1, [&](hipStream_t s, const BeamArgs& a) {
                           hipLaunchKernelGGL(ctc_lexbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, lx);
                       });
}

size_t sctc_ctc_nnbeam_workspace_bytes(const sctc_nnbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_nn(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_nnbeam_decode_batch(const sctc_nnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                 int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_nn(cfg, pl));
    NNArgs nn{};
    nn.m = cfg->lm->dev;
    return launch_beam("nnbeam", view_of(*cfg), pl,
                       BeamIO{probs_dev, ids_dev, lengths_dev, scores_dev, workspace_dev, workspace_bytes, stream},
                       cfg->sym_word, true, -1, [&](hipStream_t s, const BeamArgs& a) {
                           hipLaunchKernelGGL(ctc_nnbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, nn);
                       });
}

size_t sctc_ctc_rnnbeam_workspace_bytes(const sctc_rnnbeam_config* cfg)
{
    BeamPlan pl;
    if (plan_rnn(cfg, pl) != SCTC_OK) return 0;
    return pl.total;
}

int sctc_ctc_rnnbeam_decode_batch(const sctc_rnnbeam_config* cfg, const void* probs_dev, int32_t* ids_dev,
                                  int32_t* lengths_dev, double* scores_dev, void* workspace_dev,
                                  size_t workspace_bytes, void* stream)
{
    BeamPlan pl;
    SCTC_TRY(plan_rnn(cfg, pl));
    RNNArgs nn{};
    nn.m = cfg->lm->dev;
    nn.state_copies = 1;
    if (const char* e = getenv("SCTC_RNNBEAM_STATE_COPIES")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 4) nn.state_copies = v;
    }
    return launch_beam("rnnbeam", view_of(*cfg), pl,
                       BeamIO{probs_dev, ids_dev, lengths_dev, scores_dev, workspace_dev, workspace_bytes, stream},
                       cfg->sym_word, true, cfg->lm->device, [&](hipStream_t s, const BeamArgs& a) {
                           hipLaunchKernelGGL(ctc_rnnbeam_kernel, dim3(cfg->B), dim3(NT), 0, s, a, nn);
                       });
}

}  // extern "C"
