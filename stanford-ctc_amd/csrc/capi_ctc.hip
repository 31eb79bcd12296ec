// C ABI: library housekeeping + the CTC entry points of include/sctc.h.
#include <math.h>

#include <atomic>
#include <vector>

#include "common.h"
#include "ctc_kernels.h"

namespace sctc {

char* err_buf()
{
    static thread_local char buf[512] = {0};
    return buf;
}

int set_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// Step 1 and 2 of a call: the argument checks, then the plan (ctc_plan.h) under the switches of the environment -- read
// here, once per call.
static int ctc_check_and_plan(int B, int A, int blank, int dtype, const int32_t* T_b, const int32_t* U_b, CtcPlan* plan)
{
    SCTC_CHECK_ARG(B >= 1, "ctc: empty batch");
    SCTC_CHECK_ARG(A >= 1, "ctc: alphabet size %d < 1", A);
    SCTC_CHECK_ARG(blank >= 0 && blank < A, "ctc: blank id %d outside the alphabet", blank);
    int max_L = 0, max_T = 0;
    for (int b = 0; b < B; ++b) {
        SCTC_CHECK_ARG(T_b[b] >= 1, "ctc: utterance %d has no frames", b);
        // U == 0 is undefined behaviour in the reference (out-of-bounds read)
        SCTC_CHECK_ARG(U_b[b] >= 1, "ctc: utterance %d has an empty label sequence", b);
        max_L = std::max(max_L, 2 * U_b[b] + 1);
        max_T = std::max(max_T, T_b[b]);
    }
    *plan = ctc_plan({B, A, dtype, max_L, max_T}, ctc_switches_from_env());
    return SCTC_OK;
}

int ctc_workspace_bytes(int B, int A, int blank, int dtype, const int32_t* T_b, const int32_t* U_b, size_t* bytes)
{
    CtcPlan plan;
    SCTC_TRY(ctc_check_and_plan(B, A, blank, dtype, T_b, U_b, &plan));
    *bytes = ctc_layout(plan, T_b, U_b).bytes;
    return SCTC_OK;
}

// `keep` (optional): caller-owned host staging that outlives the async uploads; without
// it the function synchronises the stream before its local staging goes away.
struct CtcHostStage {
    std::vector<CtcUtt> utts;
    std::vector<int32_t> labels;    // the labels slice of CtcLayout
    std::vector<int32_t> cursor;
    // a kept stage (the BRNN engine's) uploads from pinned memory: the descriptors go up in the middle of a
    // step, between the forward pass and the lattice kernel (common.h, PinnedStage)
    PinnedStage pinned;
};

// Steps 3 and 4: lay the workspace out (ctc_layout), fill and upload descriptors and labels, launch what the plan names.
template <typename R>
static int run_ctc(const sctc_ctc_batch* bt, const CtcPlan& plan, const R* probs, R* grad,
                   double* cost, int32_t* skip, void* ws, size_t ws_bytes, hipStream_t stream,
                   CtcHostStage* keep)
{
    // no caller-owned stage (the standalone sctc_ctc_loss_batch): a per-thread stage that lives as long as the
    // process (never destroyed: its pinned buffer and event must not be freed behind the HIP runtime's back at exit),
    // so these uploads come from pinned memory too -- from pageable vectors the 4 MB of descriptors of a
    // 4096-utterance batch cost 1 ms with the stream waiting
    static thread_local CtcHostStage* tls_stage = new CtcHostStage();
    CtcHostStage& st = keep ? *keep : *tls_stage;
    st.utts.resize(plan.B);
    std::vector<CtcUtt>& utts = st.utts;
    const CtcLayout lay = ctc_layout(plan, bt->T_b, bt->U_b, utts.data());
    if (lay.bytes > ws_bytes)
        return set_error(SCTC_ERR_WORKSPACE, "ctc: workspace %zu bytes < %zu needed", ws_bytes, lay.bytes);
    char* const base = static_cast<char*>(ws);
    CtcUtt* d_utts = reinterpret_cast<CtcUtt*>(base + lay.utts);
    int32_t* d_labels = reinterpret_cast<int32_t*>(base + lay.labels);

    const int64_t n_int = 2 * lay.n_labels + (int64_t)plan.B * (plan.A + 1);
    st.labels.resize(n_int);
    std::vector<int32_t>& labels = st.labels;
    for (int b = 0; b < plan.B; ++b) {
        CtcUtt& u = utts[b];
        u.row0 = bt->frame_off[b];
        const int32_t* src = bt->labels + bt->label_off[b];
        for (int i = 0; i < u.U; ++i) {
            SCTC_CHECK_ARG(src[i] >= 0 && src[i] < plan.A, "ctc: label %d of utterance %d is %d, "
                           "outside the alphabet [0,%d)", i, b, src[i], plan.A);
            labels[u.lab_off + i] = src[i];
        }
        // stable counting sort of the label positions by label value: the gradient kernel sums a label's states
        // in ascending order (ctc_fast.pyx:120-131) without scanning the whole row for every label
        int32_t* start = labels.data() + 2 * lay.n_labels + (int64_t)b * (plan.A + 1);
        int32_t* grouped = labels.data() + lay.n_labels + u.lab_off;
        std::fill(start, start + plan.A + 1, 0);
        for (int i = 0; i < u.U; ++i) ++start[src[i] + 1];
        for (int k = 0; k < plan.A; ++k) start[k + 1] += start[k];
        st.cursor.assign(start, start + plan.A);
        for (int i = 0; i < u.U; ++i) grouped[st.cursor[src[i]]++] = 2 * i + 1;
    }
    const size_t utt_bytes = sizeof(CtcUtt) * plan.B, utt_span = align256(utt_bytes), lab_bytes = sizeof(int32_t) * n_int;
    char* pin = static_cast<char*>(st.pinned.acquire(utt_span + lab_bytes));
    const bool staged_pinned = pin != nullptr;
    if (pin) {
        memcpy(pin, utts.data(), utt_bytes);
        memcpy(pin + utt_span, labels.data(), lab_bytes);
        PinnedUploadGuard guard(stream, true);
        SCTC_HIP_TRY(hipMemcpyAsync(d_utts, pin, utt_bytes, hipMemcpyHostToDevice, stream));
        SCTC_HIP_TRY(hipMemcpyAsync(d_labels, pin + utt_span, lab_bytes, hipMemcpyHostToDevice, stream));
        SCTC_HIP_TRY(st.pinned.uploaded(stream));
        guard.done();
    } else {
        SCTC_HIP_TRY(hipMemcpyAsync(d_utts, utts.data(), utt_bytes, hipMemcpyHostToDevice, stream));
        SCTC_HIP_TRY(hipMemcpyAsync(d_labels, labels.data(), lab_bytes, hipMemcpyHostToDevice, stream));
    }

    if (plan.path == CTC_FUSED || plan.path == CTC_WIDE) {
        CtcFusedArgs<R> fa;
        fa.utts = d_utts;
        fa.probs = probs;
        fa.grad = grad;
        fa.ld = bt->ld;
        fa.A = plan.A;
        fa.blank = bt->blank;
        fa.rowbase = bt->rowbase_dev;
        fa.labels = d_labels;
        fa.by_label = d_labels + lay.n_labels;
        fa.label_start = d_labels + 2 * lay.n_labels;
        fa.store = base + lay.store;
        fa.cost = cost;
        fa.skip = skip;
        {
            // timing decomposition of the fused kernel (tools/ctc_diag_timing.py): parts of the schedule are switched
            // off and the results are WRONG -- never silently
            fa.diag = plan.diag;
            static std::atomic<bool> warned{false};
            if (fa.diag != 0 && !warned.exchange(true))
                fprintf(stderr, "sctc: SCTC_CTC_DIAG=%d is set: the fused CTC kernel skips parts of its schedule, costs and "
                                "gradients are WRONG (diagnostic timing runs only; unset it)\n", fa.diag);
        }
        fa.sync = plan.path == CTC_WIDE ? reinterpret_cast<uint32_t*>(base + lay.sync) : nullptr;
        if (plan.path == CTC_WIDE) SCTC_TRY(launch_ctc_fusedw<R>(fa, plan, stream));
        else SCTC_TRY(launch_ctc_fused<R>(fa, plan, stream));
    } else {
        CtcLatticeArgs<R> la;
        la.utts = d_utts;
        la.probs = probs;
        la.ld = bt->ld;
        la.A = plan.A;
        la.blank = bt->blank;
        la.lp = plan.lp;
        la.rowbase = bt->rowbase_dev;
        la.labels = d_labels;
        la.alpha = reinterpret_cast<double*>(base + lay.alpha);
        la.beta = reinterpret_cast<double*>(base + lay.beta);
        la.ll = reinterpret_cast<double*>(base + lay.ll);
        la.skip2 = reinterpret_cast<int32_t*>(base + lay.skip2);
        la.scratch = plan.path == CTC_GENERIC ? reinterpret_cast<double*>(base + lay.scratch) : nullptr;

        CtcGradArgs<R> ga;
        ga.utts = d_utts;
        ga.probs = probs;
        ga.grad = grad;
        ga.ld = bt->ld;
        ga.A = plan.A;
        ga.blank = bt->blank;
        ga.lp = plan.lp;
        ga.rowbase = bt->rowbase_dev;
        ga.labels = d_labels;
        ga.by_label = d_labels + lay.n_labels;
        ga.label_start = d_labels + 2 * lay.n_labels;
        ga.alpha = la.alpha;
        ga.beta = la.beta;
        ga.ll = la.ll;
        ga.skip2 = la.skip2;
        ga.cost = cost;
        ga.skip = skip;
        ga.lazy = plan.lazy;
        if (plan.path == CTC_GENERIC) {
            SCTC_TRY(launch_ctc_generic<R>(la, ga, plan, stream));
        } else {
            SCTC_TRY(launch_ctc_lattice<R>(la, plan, stream));
            SCTC_TRY(launch_ctc_grad<R>(ga, plan, stream));
        }
    }
    if (!staged_pinned) SCTC_HIP_TRY(hipStreamSynchronize(stream));   // pageable staging must outlive the copies
    return SCTC_OK;
}

int ctc_run_batch(const sctc_ctc_batch* bt, const void* probs, void* grad, double* cost,
                  int32_t* skip, void* ws, size_t ws_bytes, hipStream_t stream, void* keep_stage)
{
    CtcHostStage* keep = static_cast<CtcHostStage*>(keep_stage);
    SCTC_CHECK_ARG(bt && probs && grad && cost && skip, "ctc: null argument");
    SCTC_CHECK_ARG(bt->dtype == SCTC_F32 || bt->dtype == SCTC_F64, "ctc: bad dtype %d", bt->dtype);
    SCTC_CHECK_ARG(bt->ld >= bt->A, "ctc: ld %lld < A %d", (long long)bt->ld, bt->A);
    CtcPlan plan;
    SCTC_TRY(ctc_check_and_plan(bt->B, bt->A, bt->blank, bt->dtype, bt->T_b, bt->U_b, &plan));
    if (bt->dtype == SCTC_F32)
        return run_ctc<float>(bt, plan, (const float*)probs, (float*)grad, cost, skip, ws,
                              ws_bytes, stream, keep);
    return run_ctc<double>(bt, plan, (const double*)probs, (double*)grad, cost, skip, ws,
                           ws_bytes, stream, keep);
}

void* ctc_new_stage() { return new CtcHostStage(); }
void ctc_free_stage(void* p) { delete static_cast<CtcHostStage*>(p); }

}  // namespace sctc

using namespace sctc;

extern "C" {

int sctc_abi_version(void) { return SCTC_ABI_VERSION; }

const char* sctc_last_error(void) { return err_buf(); }

int sctc_set_device(int device)
{
    SCTC_HIP_TRY(hipSetDevice(device));
    return SCTC_OK;
}

int sctc_device_info(int* compute_units, int* lds_bytes_per_cu, int64_t* total_mem_bytes,
                     char* name, int name_len)
{
    int dev = 0;
    SCTC_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    SCTC_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (total_mem_bytes) *total_mem_bytes = (int64_t)prop.totalGlobalMem;
    if (name && name_len > 0) {
        snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    return SCTC_OK;
}

size_t sctc_ctc_workspace_bytes(const sctc_ctc_batch* bt)
{
    if (!bt) return 0;
    size_t bytes = 0;
    if (ctc_workspace_bytes(bt->B, bt->A, bt->blank, bt->dtype, bt->T_b, bt->U_b, &bytes) != SCTC_OK) return 0;
    return bytes;
}

int sctc_ctc_loss_batch(const sctc_ctc_batch* batch, const void* probs_dev, void* grad_dev,
                        double* cost_dev, int32_t* skip_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream)
{
    return ctc_run_batch(batch, probs_dev, grad_dev, cost_dev, skip_dev, workspace_dev,
                         workspace_bytes, (hipStream_t)stream, nullptr);
}

int sctc_softmax_rows(const float* logits_dev, float* probs_dev, int64_t rows, int32_t A,
                      int64_t ld, void* stream)
{
    SCTC_CHECK_ARG(logits_dev && probs_dev, "softmax_rows: null pointer");
    return launch_softmax_rows(logits_dev, probs_dev, rows, A, ld, (hipStream_t)stream);
}

int sctc_argmax_rows(const void* probs_dev, int32_t dtype, int32_t* best_dev, int64_t rows,
                     int32_t A, int64_t ld, void* stream)
{
    SCTC_CHECK_ARG(probs_dev && best_dev, "argmax_rows: null pointer");
    return launch_argmax_rows(probs_dev, dtype, best_dev, rows, A, ld, (hipStream_t)stream);
}

}  // extern "C"
