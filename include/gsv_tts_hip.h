/*
 * gsv_tts_hip.h -- C ABI of the MI355X (gfx950) GPT-SoVITS inference hot path.
 *
 * The reference (chinokikiss/GSV-TTS-Lite) has no FFI: its hot path is PyTorch modules
 * driven from Python.  This header is the boundary a maintainer would bind underneath those
 * modules (ctypes stub in INTEGRATION.md).  Every entry point names the reference interface
 * it replaces (file:line in the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types; returns GSV_OK (0) or an
 *     error code, message via gsv_last_error() (thread-local).  No exceptions cross the ABI.
 *   - All tensor pointers are DEVICE pointers unless a parameter says "host".
 *   - `stream` is a hipStream_t passed as void* (torch: torch.cuda.current_stream().cuda_stream).
 *   - Ownership mirrors the reference: the caller owns KV caches, kv_len and
 *     every I/O buffer (torch allocations made once in initialize_runtime); the library owns
 *     only its repacked weight arena and fixed scratch, created at load time.  Nothing is
 *     allocated or freed inside a step, so steps are hipGraph-capturable.
 *   - One caller per handle at a time (the reference serialises with TTS._infer_lock,
 *     gsv_tts/TTS.py:145); distinct handles (one per GPU/process) are independent.
 */
#ifndef GSV_TTS_HIP_H
#define GSV_TTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSV_OK 0
#define GSV_ERR_ARG 1     /* bad argument / unknown tensor name / shape mismatch */
#define GSV_ERR_HIP 2     /* a HIP runtime call failed */
#define GSV_ERR_STATE 3   /* call order violated (e.g. step before finalize/bind) */

#define GSV_F32 0         /* fp32 weights/KV/activations: the bit-exact-token parity mode */
#define GSV_BF16 1        /* bf16 weights + KV (+ bf16 vocoder activations), fp32 accumulate */
#define GSV_FP8 2         /* gsv_t2s only: GSV_BF16 plus OCP e4m3 QKV / FFN weights (per-output-channel scale) and e4m3
                             activations on the fp8 MFMA in the batched decode step; K/V cache, out-proj, prefill: bf16 */

int gsv_version(void);
const char* gsv_last_error(void);

/* ------------------------------------------------------------------------------------------
 * GPT semantic-token decoder  (reference: gsv_tts/GPT_SoVITS/GPT/t2s_model.py)
 * ---------------------------------------------------------------------------------------- */
typedef struct gsv_t2s gsv_t2s;

typedef struct {
    int n_layer, hidden, n_head, vocab, eos; /* config["model"], t2s_model.py:159-168 */
    int n_pos;                               /* rows of the sinusoidal tables (4000, t2s_model.py:212) */
    int n_phoneme;                           /* phoneme_vocab_size */
    int dtype;                               /* GSV_F32 | GSV_BF16 | GSV_FP8 */
} gsv_t2s_config;

/* replaces Text2SemanticDecoder.__init__ + Loader.get_gpt_weights (gsv_tts/Loader.py:111-170) */
int gsv_t2s_create(const gsv_t2s_config* cfg, gsv_t2s** out);
int gsv_t2s_destroy(gsv_t2s* h);

/* Hand one fp32 device tensor to the library under its reference state-dict name (after the
 * Loader.py:130-154 remap), e.g. "t2s_transformer.blocks.3.qkv.weight", "ar_predict_layer.weight",
 * "ar_audio_embedding.word_embeddings.weight", "bert_proj.weight".  Two synthetic names carry
 * the host-precomputed tables alpha*pe of embedding.py:58-69: "ar_text_position.pe_scaled",
 * "ar_audio_position.pe_scaled" ([n_pos][hidden]).  The data is converted/repacked into the
 * library's arena during the call (stream-ordered); the source may be freed afterwards. */
int gsv_t2s_load_tensor(gsv_t2s* h, const char* name, const float* data, int64_t numel, void* stream);
/* all tensors present?  builds decode panels; required before any step */
int gsv_t2s_finalize(gsv_t2s* h, void* stream);

/* Caller-owned runtime state for ONE batch size: the reference's Bucket family for that batch
 * size (t2s_model.py:146-156, 240-276).  All bucket lengths of a batch size alias one storage
 * with the largest T as stride, so `max_kv` is that largest T ("nested" KV cache). */
typedef struct {
    int batch;              /* B */
    int max_kv;             /* T: positions per sequence (cache stride) */
    void* k_cache;          /* [n_layer][B][n_head][T][head_dim], cfg.dtype */
    void* v_cache;          /* same */
    int64_t* kv_len;        /* [B]   Bucket.kv_cache_len */
    int64_t* x_len;         /* [B]   text length per slot (PE offset, t2s_model.py:456,728) */
    int64_t* pre_tokens;    /* [B][T+1] sampled token at kv position (t2s_model.py:605,653); column T
                               holds the sample taken when the cache is exactly full */
    uint8_t* seen;          /* [B][vocab] repetition-penalty membership (prompt + generated) */
    int32_t* step;          /* [B]   logits launches since the slot was (re)filled */
    int32_t* eos_at;        /* [B]   first step whose sample was EOS, else -1 */
    float* logits;          /* [B][vocab] last logits after suppression/penalty (host sampling) */
    float* hidden;          /* [B][hidden] last final hidden state (Bucket.graph_xy_dec) */
    int64_t* tok_override;  /* [B]   host-sampled tokens, consumed when ctl[0] == 1; with ctl[0] == 2 (device sampling) a value
                               v > 0 makes v - 1 the sequence's noise stream instead of its slot index (key it by request
                               and a request's samples do not depend on slot, refill order or rank) */
    int32_t* ctl;           /* [8]   {sample_mode, suppress_steps, rep_enabled, -, top_k, seed_lo, seed_hi,
                               suppress_first}; suppress_first != 0: the prefill's sample never takes 280 / 486 / EOS
                               (infer / infer_stream, t2s_model.py:415-416), independent of suppress_steps; sample_mode 0 = greedy argmax, 1 = tok_override (host sampling),
                               2 = device sampling: temperature fctl[1], top-k ctl[4] (<= 0: off; ties with the
                               k-th value are kept, GPT/utils.py:45-48), then argmax(softmax / Exp(1))
                               (utils.py:56-59) with a counter-based noise stream keyed by
                               (seed, slot, kv position, step, token id); top-p fctl[2] in (0,1) is applied first, on the
                               un-tempered logits, as the set {p >= tau} (ties with tau stay together) */
    float* fctl;            /* [4]   {repetition_penalty, temperature, top_p, -} */
} gsv_t2s_state;
int gsv_t2s_bind_state(gsv_t2s* h, const gsv_t2s_state* st);
/* Forgets the state bound for `batch`: its captured steps are destroyed and its staging goes back to the handle, so the caller may
 * free the tensors the state pointed at (the reference rebuilds its runtime the same way: initialize_runtime, t2s_model.py:210-298,
 * drops the old buckets).  The caller makes sure nothing of that state is still running.  Unknown batch: GSV_OK. */
int gsv_t2s_unbind_state(gsv_t2s* h, int batch);
/* Optional: `host_mapped` [batch] int32 in host memory the device can write (hipHostMalloc / a pinned torch tensor), or
 * NULL to turn it off.  Every kernel that sets state.eos_at[slot] then also publishes the value there (system-scope store),
 * so the host loop of t2s_model.py:451-453 reads the EOS flag from its own memory after an event instead of enqueuing a
 * device-to-host copy between the decode windows.  Call after gsv_t2s_bind_state (which clears it); it invalidates the
 * captured steps of this batch size. */
int gsv_t2s_set_eos_mirror(gsv_t2s* h, int batch, int32_t* host_mapped);

/* Optional: PER-SLOT sampling parameters for one bound state (continuous batching whose requests bring their own top_k / top_p /
 * temperature / seed; the reference's batched loop has one set per call, t2s_model.py:555-734).  `table` is a caller-owned DEVICE
 * array of `batch` entries, 16-byte aligned, or NULL to turn it off.  With a table the token step takes slot b's sample_mode
 * (0 greedy | 2 device sampling) and parameters from table[b] instead of ctl[0], ctl[4..6], fctl[1..2], and the logits kernel --
 * of every step AND of every prompt pass that runs in this state -- takes slot b's repetition penalty, suppress_steps and
 * first-sample suppression from table[b] instead of fctl[0], ctl[1], ctl[7] (first-sample suppression is on iff suppress_steps
 * > 0; the penalty is applied iff rep_penalty is neither 0 nor 1, whatever ctl[2] says).  What stays in ctl: ctl[0] == 1 (host
 * tokens), a whole-state mode that overrides the table, and ctl[2], the whole-state switch "keep `seen` up to date": set it when
 * any request that may run in the state penalises (the token step then records every live slot's tokens in its `seen` row).
 * The entries are read from device memory by every step, so one captured step serves any mix and an entry may change between two
 * gsv_t2s_decode calls.
 * ORDER.  The prompt pass's logits are penalised and suppressed, so a request's entry AND its `seen` row (gsv_t2s_seed_seen) have
 * to be in place in the state where its PROMPT PASS runs, before that pass: the stepped state for gsv_t2s_prefill /
 * gsv_t2s_prefill_slots / gsv_t2s_prefill_slots_staged into a parked slot (the steps leave a parked slot's `seen` row alone), the
 * ahead state's own table and `seen` for a pass that gsv_t2s_adopt_slots moves later.  The slot's pending token is drawn by the
 * token kernel of the next step (or gsv_t2s_flush) of the state the slot lives in, so after gsv_t2s_adopt_slots (which carries
 * the `seen` row, not the entry) the entry is put into the adopting state's table as well, before its next step.
 * gsv_t2s_commit_slots needs nothing; gsv_t2s_move_slots carries a moved slot's entry and `seen` row to the destination
 * (GSV_ERR_ARG when the source has a table and the destination has none).  GSV_STEP_FUSED_TOKEN keeps its meaning: the caller's
 * promise that no slot samples.  Call after gsv_t2s_bind_state (which clears it); a change of the table pointer invalidates the
 * captured steps of this batch size. */
typedef struct {
    int32_t sample_mode;    /* 0 greedy argmax | 2 device sampling */
    int32_t top_k;          /* as ctl[4] */
    float temperature;      /* as fctl[1] */
    float top_p;            /* as fctl[2] */
    int32_t seed_lo, seed_hi; /* as ctl[5], ctl[6]; the noise stream stays tok_override[slot] - 1, else the slot index */
    float rep_penalty;      /* as fctl[0] with ctl[2] set; 0 (or 1): no penalty, the slot's logits are left bit for bit */
    int32_t suppress_steps; /* as ctl[1], and > 0 also as ctl[7]: the prompt pass's sample and every sample while step <
                               suppress_steps never take 280 / 486 / EOS; 0: no suppression */
} gsv_t2s_slot_sampling;
int gsv_t2s_set_slot_sampling(gsv_t2s* h, int batch, gsv_t2s_slot_sampling* table);
/* Writes table[slots[r]] = entries[r] on `stream`; slots / entries are HOST arrays [nrows] that ride in the kernel arguments (no
 * host-to-device copy between two decode windows).  GSV_ERR_STATE without a table; GSV_ERR_ARG for a slot out of range, a
 * sample_mode other than 0 / 2, a negative or non-finite rep_penalty or negative suppress_steps. */
int gsv_t2s_put_slot_sampling(gsv_t2s* h, int batch, const int32_t* slots, const gsv_t2s_slot_sampling* entries, int nrows,
                              void* stream);

/* The repetition-penalty set of slots that take a request, in ONE launch on `stream`: for each row r, seen[slots[r]] is cleared
 * and then seen[slots[r]][t] = 1 for every t in tokens[offsets[r] .. offsets[r + 1]) (the request's prompt tokens, which the
 * reference penalises together with the generated ones, t2s_model.py:418-420; ids outside [0, vocab) are ignored).  slots
 * [nrows <= 64, distinct] and offsets [nrows + 1, non-decreasing] are HOST arrays that ride in the kernel arguments; tokens is a
 * packed DEVICE array (may be NULL when no row has tokens).  A row without tokens only clears: that is how a slot whose new
 * request does not penalise gets rid of its previous tenant's set.  Call it before the request's prompt pass, in the state and on
 * the stream that pass runs in (see gsv_t2s_set_slot_sampling: ORDER). */
int gsv_t2s_seed_seen(gsv_t2s* h, int batch, const int32_t* slots, const int64_t* tokens, const int32_t* offsets, int nrows,
                      void* stream);

/* replaces process_single_data / process_batch_data (t2s_model.py:300-383): builds packed rows
 * [x_b | y_b | 0-pad] = text-emb + bert_proj + alpha_t*pe, audio-emb + alpha_a*pe.
 *   x_ids [nrows][lx_max], y_ids [nrows][ly_max], bert [nrows][lx_max][1024] (row-padded),
 *   x_lens/y_lens [nrows] -> xy [nrows][l_max][hidden] fp32.  scratch: [nrows*lx_max][hidden] f32 */
int gsv_t2s_embed_prompt(gsv_t2s* h, int nrows, int lx_max, int ly_max, int l_max, const int64_t* x_ids,
                         const int64_t* y_ids, const float* bert, const int64_t* x_lens,
                         const int64_t* y_lens, float* xy, float* scratch, void* stream);

/* replaces T2STransformer.process_prompt (t2s_model.py:31-65,114-127) + ar_predict_layer +
 * the first sample (t2s_model.py:414-420, 608-616).  xy [nrows][l_max][hidden] is consumed
 * (overwritten with the hidden states).  Attention mask is the reference's prompt mask,
 * implied by (x_len, y_len) per row: text rows see all text, audio rows see all text + causal
 * audio; rows/cols >= x_len+y_len are padding.  K/V for positions [0, x_len+y_len) go to cache
 * rows slot0..slot0+nrows-1 of the state bound for `batch`; afterwards for those slots:
 * kv_len = x_len + y_len, x_len set, step = 0, eos_at = -1, and the first token is pending
 * (sampled from logits[:, :-1], i.e. EOS impossible; suppression per ctl).
 * workspace: gsv_t2s_prefill_workspace(h, nrows, l_max) bytes. */
size_t gsv_t2s_prefill_workspace(gsv_t2s* h, int nrows, int l_max);
int gsv_t2s_prefill(gsv_t2s* h, int batch, int slot0, int nrows, int l_max, float* xy, const int64_t* x_lens,
                    const int64_t* y_lens, void* workspace, size_t workspace_bytes, void* stream);
/* The same for rows that go to scattered slots (the continuous-batching refill of every sequence that finished in a
 * check window, t2s_model.py:696-722, as ONE packed prefill): slots int32 [nrows] on the device, distinct, each
 * < batch; row r fills slot slots[r]. */
int gsv_t2s_prefill_slots(gsv_t2s* h, int batch, const int32_t* slots, int nrows, int l_max, float* xy, const int64_t* x_lens,
                          const int64_t* y_lens, void* workspace, size_t workspace_bytes, void* stream);

/* The refill as an ASYNCHRONOUS pair, for continuous batching that does not stall its decode steps on a prompt pass:
 *   gsv_t2s_prefill_slots_staged  the same prompt pass, callable on ANOTHER stream than the one the decode step
 *       replays on.  It writes the K/V rows [0, x_len + y_len) of the listed slots and puts everything else the
 *       step also writes (kv_len, x_len, step, eos_at, the first logits / hidden / pending token) into the library's
 *       staging of that batch size.  Contract: before calling, PARK each listed slot by setting kv_len[slot] = -1
 *       on the step's stream and treat it as idle: the decode step keeps a parked slot parked, sends its K/V row to the
 *       last row of the cache (which no prompt of <= max_kv - 1 positions uses), lets it attend over row 0 only and
 *       leaves its `seen` set alone.
 *   gsv_t2s_commit_slots  on the step's stream, once the staged pass has completed (event): staging -> live state of
 *       the listed slots; the next step decodes them.  Rows are independent, so tokens per request are unchanged. */
int gsv_t2s_prefill_slots_staged(gsv_t2s* h, int batch, const int32_t* slots, int nrows, int l_max, float* xy,
                                 const int64_t* x_lens, const int64_t* y_lens, void* workspace, size_t workspace_bytes,
                                 void* stream);
int gsv_t2s_commit_slots(gsv_t2s* h, int batch, const int32_t* slots, int nrows, void* stream);

/* Prompt passes AHEAD of the slots that will decode them (continuous batching whose refills cost no idle slot-steps; the
 * reference prefills a request when a slot has finished, t2s_model.py:696-722, and every slot waits for it).  Bind a SECOND
 * state of another batch size (`batch_src`, with a KV cache of its own, never stepped) and run the prompt passes of the
 * NEXT requests into it with gsv_t2s_prefill_slots_staged on a side stream, several requests per pass, while the steps of
 * `batch_dst` run.  When a slot of `batch_dst` has finished, this call -- on the step's stream, after the pass's completion
 * event -- copies K/V rows [0, kv_len) of source slot slots_src[r] into slot slots_dst[r] and moves the staged kv_len,
 * x_len, step, eos_at, first logits / hidden / pending token into the live state of slots_dst[r], and the source slot's `seen`
 * row (the set the pass penalised its first sample against) into seen[slots_dst[r]]; the next step decodes it.
 * slots_dst / slots_src / tok_override are HOST arrays [nrows] (they ride in the kernel arguments); tok_override (may be
 * NULL) sets state.tok_override[slots_dst[r]] (device sampling: the request's noise stream).  A prompt pass is
 * row-independent and packing-invariant, so a request's tokens do not depend on when or beside what it was prefilled. */
int gsv_t2s_adopt_slots(gsv_t2s* h, int batch_dst, const int32_t* slots_dst, int batch_src, const int32_t* slots_src,
                        const int64_t* tok_override, int nrows, void* stream);

/* Tail compaction of the slot loop (the reference lets finished slots "keep decoding garbage" once its queue is empty,
 * t2s_model.py:684-694: the last requests then pay the step of the full batch size).  Moves LIVE slots of one stepped state into
 * slots of ANOTHER bound state with a KV cache of its own (max_kv >= the source's) between two steps, on the step's stream:
 * K/V rows [0, kv_len), kv_len, x_len, the token history (pre_tokens), the repetition-penalty set (seen), step, eos_at,
 * tok_override and what the next step reads of the previous one (logits, hidden, pending token).  The next gsv_t2s_decode of
 * `batch_dst` continues every moved request where `batch_src` left it.  slots_dst / slots_src are HOST arrays [nrows <= 64];
 * a slot may be listed once per side.  Slots of `batch_dst` that are not listed keep their state (park them with kv_len = -1). */
int gsv_t2s_move_slots(gsv_t2s* h, int batch_dst, const int32_t* slots_dst, int batch_src, const int32_t* slots_src, int nrows,
                       void* stream);

/* replaces T2STransformer.decode_next_token (t2s_model.py:67-105,129-143) for an EXPLICIT input
 * x [B][hidden] (parity seam): appends K/V at kv_len[b], attends to [0, kv_len[b]], writes the
 * final hidden state to state.hidden and bumps kv_len.  No sampling.  Takes the path gsv_t2s_decode would take for
 * this batch size (per-sequence kernels, or the batched chain from gsv_t2s_batched_min sequences on). */
int gsv_t2s_decode_hidden(gsv_t2s* h, int batch, const float* x, void* stream);

/* The AR hot loop body (t2s_model.py:430-456 / 637-653, 727-728) `n_steps` times, all on device:
 * take the pending token (greedy argmax of the penalised logits, or tok_override), record it in
 * pre_tokens[b][kv_len[b]], build emb + alpha*pe[kv_len - x_len], run the layers, bump kv_len,
 * compute the next logits (suppression while step < ctl[1]; repetition penalty over `seen`).
 * `use_graph` is a bit set: GSV_STEP_GRAPH replays the step from a hipGraph captured on first use (one per batch size and
 * flag combination); GSV_STEP_FUSED_TOKEN is the caller's promise that ctl[0] is 0 or 1 (greedy or tok_override, i.e. no
 * device sampling) for these steps -- on the two-launches-per-layer path (below the batched chain's size) the first layer's
 * attention kernel then does the token kernel's work itself (one launch less per step; same tokens, same state).
 * From a tuned batch size on (bf16 / fp8 handles) the step is the batched chain of csrc/t2s_batch.h: weights
 * streamed once per step through MFMA GEMMs instead of once per sequence. */
#define GSV_STEP_GRAPH 1
#define GSV_STEP_FUSED_TOKEN 2
int gsv_t2s_decode(gsv_t2s* h, int batch, int n_steps, int use_graph, void* stream);
/* Batch size from which gsv_t2s_decode runs the batched chain (INT_MAX on fp32 handles: never).  Tests mirror the
 * choice in the oracle, whose reduced-precision modes round the operands each path rounds. */
int gsv_t2s_batched_min(gsv_t2s* h);
/* FFN slices per sequence of the two-launches-per-layer step at this batch size: 32 slices of 64 hidden units, or -- at
 * <= 4 sequences -- 64 slices of 32 (fp32 handles too: their partials stay fp32).  Each slice's partial 512-vector crosses the kernel boundary rounded to half on
 * bf16 handles, so the count is part of the arithmetic; the bf16-mode oracle sums the same slices (oracle.py). */
int gsv_t2s_ffn_slices(gsv_t2s* h, int batch);
/* Device memory the handle owns, in bytes (its arena's blocks: repacked weights, fragments, scratch, the staging of every
 * bound state).  Pieces given back inside the handle -- a state re-bound with gsv_t2s_bind_state, a tensor re-loaded with
 * gsv_t2s_load_tensor, scratch that grew -- are handed out again by size, so re-binding the same shapes or hot-swapping
 * weights of the same architecture for a handle's whole life leaves this number where it was; all of it is released by
 * gsv_t2s_destroy. */
size_t gsv_t2s_device_bytes(gsv_t2s* h);
/* Measurement aid (bench.py `roofline`): average time in ms of ONE launch of each per-sequence decode-step
 * kernel class {attn, ffn, logits, token}: the class's launches over all layers (every layer streams its own
 * weights, as in a real step) are captured into a hipGraph and replayed `iters` times between two hipEvents on
 * `stream` -- no host launch cost, but the dependent-launch gap every kernel of a real step pays is included.
 * out_ms: host float[4].  kv_len is left untouched; the sweeps rewrite the K/V row AT kv_len, the pending
 * token's pre_tokens / seen / eos_at entries and the partial-sum scratch, all of which the next real step
 * (or prefill) overwrites -- call it between utterances, not inside one. */
int gsv_t2s_time_kernels(gsv_t2s* h, int batch, int iters, float* out_ms, void* stream);
/* Bring-up aid: when `buf` (device, >= 64 x uint64) is non-null the LAST layer's attn/ffn kernels
 * write shader-clock timestamps of their phases into it (slots 0-7 attn, 8-15 ffn: the block's first wave; + 16: its last;
 * attn slot 16, behind park(): entries 32 / 33). */
int gsv_t2s_set_debug(gsv_t2s* h, void* buf);
/* materialise the pending token of every slot into pre_tokens/seen/eos_at (idempotent) */
int gsv_t2s_flush(gsv_t2s* h, int batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * SoVITS flow + Generator  (reference: gsv_tts/GPT_SoVITS/SoVITS/models.py, module/modules.py)
 * ---------------------------------------------------------------------------------------- */
typedef struct gsv_voc gsv_voc;

typedef struct {
    int inter_channels, hidden_channels, gin_channels, upsample_initial_channel;
    int n_upsample;
    int upsample_rates[8], upsample_kernel_sizes[8];
    int n_resblock_kernels;
    int resblock_kernel_sizes[4];
    int resblock_dilations[4];   /* (1,3,5): same for every resblock, modules.py:116 */
    int n_flows;                 /* 4 coupling layers, models.py:31 */
    int dtype;                   /* GSV_F32 | GSV_BF16 */
} gsv_voc_config;

/* replaces SynthesizerTrn.{flow,dec} construction + Loader.get_sovits_weights (Loader.py:59-103) */
int gsv_voc_create(const gsv_voc_config* cfg, gsv_voc** out);
int gsv_voc_destroy(gsv_voc* h);
/* fp32 device tensor under its state-dict name: "dec.*" (weight-norm removed, Loader.py:95),
 * "flow.flows.{0,2,4,6}.*" (weight_g/weight_v still separate; folded by finalize) and, optionally,
 * "enc_p.*" + "quantizer.vq.layers.0._codebook.embed" (enables gsv_voc_enc_p on bf16 handles) */
int gsv_voc_load_tensor(gsv_voc* h, const char* name, const float* data, int64_t numel, void* stream);
int gsv_voc_finalize(gsv_voc* h, void* stream);

/* replaces SynthesizerTrn.flow_dec (models.py:380-383): o = dec(flow(z_p, mask, ge) * mask, g=ge).
 *   z_p [inter][T] fp32 channels-first (torch layout), y_mask [T], ge [gin][Tg] with Tg in {1, T}
 *   (Tg == T: per-frame speaker embedding of the time-concatenated batch, TTS.py:740-744)
 *   out [T * prod(upsample_rates)] fp32.  workspace from gsv_voc_workspace(h, T). */
size_t gsv_voc_workspace(gsv_voc* h, int T);
int gsv_voc_flow_dec(gsv_voc* h, const float* z_p, const float* y_mask, const float* ge, int T, int Tg,
                     float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same pass replayed from a hipGraph captured on first use for this (z_p, y_mask, ge, out, workspace, T, Tg) --
 * the reference's per-bucket CUDA graphs of SynthesizerTrn.initialize_runtime / decode (models.py:322-369, 406-423): the
 * caller owns STATIC buffers per bucket length, copies the chunk in (zero mask beyond the real length), replays, slices.
 * A 50-frame streaming chunk is ~60 launch-bound kernels; replay removes their host launch cost. */
int gsv_voc_flow_dec_graph(gsv_voc* h, const float* z_p, const float* y_mask, const float* ge, int T, int Tg,
                           float* out, void* workspace, size_t workspace_bytes, void* stream);
/* x fp32 [C][T_in] -> y fp32 [C][T_out], linear resampling as F.interpolate(mode="linear", align_corners=False): the
 * `speed != 1` resampling of TextEncoder.infer (models.py:217-219), applied to the projected statistics (proj is 1x1
 * affine, so resampling its output equals resampling its input). */
int gsv_voc_resample_linear(const float* x, int C, int T_in, float* y, int T_out, void* stream);
/* parity seams: the flow alone (ResidualCouplingBlock.forward reverse, models.py:58-65) and the
 * Generator alone (models.py:113-132); same layouts. */
int gsv_voc_flow(gsv_voc* h, const float* z_p, const float* y_mask, const float* ge, int T, int Tg,
                 float* z_out, void* workspace, size_t workspace_bytes, void* stream);
int gsv_voc_dec(gsv_voc* h, const float* z, const float* ge, int T, int Tg, float* out, void* workspace,
                size_t workspace_bytes, void* stream);

/* enc_p on device (bf16 handles that were given the "enc_p.*" and "quantizer.vq.layers.0._codebook.embed"
 * tensors): replaces quantizer.decode + the x2 nearest upsampling + TextEncoder.infer for speed == 1,
 * non-streaming calls (SoVITS/models.py:196-224, 387-400; attentions.py:58-220; mrte_model.py:20-38).
 *   codes int64 [n_codes], text int64 [n_text], ge512 fp32 channels-LAST [Tg][512] (ge_to512(ge) for v2Pro /
 *   v2ProPlus, ge itself for v2), Tg in {1, 2*n_codes}; slice_indices int64 [2*n_codes][2] or NULL
 *   (per-frame phoneme range of the time-concatenated batch, mrte_model.py:27-33)
 *   -> m_p, logs_p fp32 [inter][T] channels-first, T = 2*n_codes; attn fp32 [4][T][n_text] or NULL
 *   (enc_p.mrte.cross_attention.attn, read by TTS for subtitles).  y_mask is all ones (batch of one). */
int gsv_voc_has_enc_p(gsv_voc* h);
size_t gsv_voc_enc_workspace(gsv_voc* h, int n_codes, int n_text);
int gsv_voc_enc_p(gsv_voc* h, const int64_t* codes, int n_codes, const int64_t* text, int n_text, const float* ge512, int Tg,
                  const int64_t* slice_indices, float* m_p, float* logs_p, float* attn, void* workspace, size_t workspace_bytes,
                  void* stream);

/* SynthesizerTrn.decode (SoVITS/models.py:385-429) as ONE call -- nothing of it is left to the caller's tensor library:
 *   codes int64 [n_codes] (n_q = 1, batch 1), text int64 [n_text];
 *   ge fp32 [gin][Tg] channels-first, Tg = 1 (one speaker) or n_codes (per-TOKEN columns of a time-concatenated batch: the
 *     x2 nearest upsampling of models.py:389 and the nearest resize of :402 are index maps inside);
 *   ge_to512 (v2Pro / v2ProPlus, :394), quantizer lookup + x2 upsampling + TextEncoder.infer (enc_p, :395-400; slice_indices as
 *     for gsv_voc_enc_p), streaming slice + cross-fade (valid_start, overlap_len > 0, overlap_state fp32 [2*inter][overlap_len]
 *     in/out, has_overlap = 0 on a stream's first chunk; module/models.py:209-215), speed resampling to `out_frames` frames
 *     (:217-219: the caller evaluates int(T' / speed) + 1 ONCE, in the arithmetic it sizes `out` with -- Python doubles in the
 *     reference -- and passes the result; out_frames == T' means speed 1, no resampling), z_p = m_p + N(0,1) * exp(logs_p) * noise_scale (:404), flow + Generator (:380-383).
 *   The noise is counter-based (lowbias32 of the element index and `seed`, Box-Muller): a call is replayable from its seed; it is
 *   not torch's generator stream.  use_graph != 0 replays flow + Generator from a hipGraph captured for this workspace
 *   (keep one workspace per chunk length: the reference's per-bucket CUDA graphs, models.py:322-369); a handle keeps at most
 *   GSV_VOC_MAX_GRAPHS captured passes and evicts the least recently replayed one.
 *   -> out fp32 [out_frames * prod(upsample_rates)], T' = 2 n_codes - valid_start;
 *      attn fp32 [4][2 n_codes][n_text] or NULL.  workspace: gsv_voc_decode_workspace(...) bytes, device. */
#define GSV_VOC_MAX_GRAPHS 64
size_t gsv_voc_decode_workspace(gsv_voc* h, int n_codes, int n_text, int Tg, int out_frames, int valid_start);
int gsv_voc_decode(gsv_voc* h, const int64_t* codes, int n_codes, const int64_t* text, int n_text, const float* ge, int Tg,
                   const int64_t* slice_indices, float noise_scale, unsigned long long seed, int out_frames, int valid_start, int overlap_len,
                   float* overlap_state, int has_overlap, int use_graph, float* out, float* attn, void* workspace, size_t workspace_bytes,
                   void* stream);

/* gsv_voc_decode over a time-concatenated batch whose utterances each have their own speed, noise scale and seed.  The
 * `n_segments` entries of `segments` (a HOST array, 1..GSV_VOC_MAX_SEGMENTS, read before the call returns) follow one another:
 * segment i covers codes [sum_{k<i} n_codes_k, + n_codes_i) -- input frames twice that -- and output frames
 * [sum_{k<i} out_frames_k, + out_frames_i); sum n_codes_i == n_codes.  out_frames_i is the caller's int(2 n_codes_i / speed_i) + 1
 * (2 n_codes_i for speed 1: copied, not resampled), evaluated once as for gsv_voc_decode.
 *   ge_to512 and enc_p run on the whole concatenation (codes, text, ge, Tg in {1, n_codes}, slice_indices: as gsv_voc_decode).
 *   Then ONE kernel writes z_p, the mask and the per-frame conditioning of all T_out = sum out_frames_i frames: each segment's
 *   [m_p | logs_p] is resampled on its own (F.interpolate(mode="linear") of its 2 n_codes_i frames, both taps clamped to the
 *   segment: no output frame blends two utterances), its noise is N(seed_i, c * out_frames_i + j) * exp(logs_p) * noise_scale_i
 *   -- what gsv_voc_decode draws for that utterance alone with that seed; noise_scale_i == 0 adds nothing -- and frame j of the
 *   segment takes the conditioning of its token min(floor(j * 2 n_codes_i / out_frames_i), 2 n_codes_i - 1) / 2.  flow +
 *   Generator then run over T_out frames.  No streaming, no hipGraph.
 *   -> out fp32 [T_out * prod(upsample_rates)]: segment i is samples [o_i, o_i + out_frames_i) * prod(upsample_rates);
 *      attn fp32 [4][2 n_codes][n_text] (INPUT frames) or NULL.  workspace: gsv_voc_decode_segments_workspace(...) bytes, device.
 * The table is checked before anything is launched: GSV_ERR_ARG, and gsv_last_error names the first bad entry, for n_segments
 * outside 1..GSV_VOC_MAX_SEGMENTS, n_codes_i < 1, out_frames_i < 1, sum n_codes_i != n_codes or Tg outside {1, n_codes}; the
 * workspace query returns 0 for the same inputs.  One segment with gsv_voc_decode's arguments gives gsv_voc_decode's samples. */
#define GSV_VOC_MAX_SEGMENTS 64
typedef struct gsv_voc_segment {
    int32_t n_codes;     /* tokens of this utterance */
    int32_t out_frames;  /* frames after its speed change */
    float noise_scale;
    uint64_t seed;       /* of its noise stream */
} gsv_voc_segment;
size_t gsv_voc_decode_segments_workspace(gsv_voc* h, int n_codes, int n_text, int Tg, const gsv_voc_segment* segments, int n_segments);
int gsv_voc_decode_segments(gsv_voc* h, const int64_t* codes, int n_codes, const int64_t* text, int n_text, const float* ge, int Tg,
                            const int64_t* slice_indices, const gsv_voc_segment* segments, int n_segments, float* out, float* attn,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Subtitle alignment: monotonic Viterbi path of vocoder frames over phonemes -- replaces
 * TTS._viterbi_monotonic (gsv_tts/TTS.py:1744-1797), which TTS.infer / infer_stream / infer_batched call on
 * the `attn` returned by vq_model.decode (TTS.py:250, 445, 769).
 *   attn fp32 [H][T][N] (device; H <= 8 heads, T frames, 2 <= N <= 4096 phonemes)
 *   -> assign int32 [T] (device): phoneme per frame, -1 before the first frame whose head-averaged attention
 *   peaks at phoneme 0.  workspace (device) from gsv_align_workspace(T, N); nothing is allocated. */
size_t gsv_align_workspace(int T, int N);
int gsv_align_viterbi(const float* attn, int H, int T, int N, int32_t* assign, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Streaming splice: replaces TTS._sola_algorithm (gsv_tts/TTS.py:1612-1627), which TTS.infer_stream calls between the decode of a
 * chunk and its hand-out (TTS.py:429-431).
 *   prev_tail fp32 [overlap]: the last `overlap` samples of the previous (already spliced) chunk; chunk fp32 [n], n >= overlap.
 *   The chunk is slid by the offset k in [0, min(n, overlap + search_len) - overlap] that maximises
 *   sum_j chunk[k + j] prev_tail[j] / sqrt(sum_j chunk[k + j]^2 + 1e-8) (first maximum), then cross-faded with
 *   alpha = linspace(0, 1, overlap):  out[i] = prev_tail[i] (1 - alpha_i) + chunk[k + i] alpha_i for i < overlap, chunk[k + i] behind.
 *   -> out fp32 (capacity n; n - *offset samples are written), offset int32 [1] (device; read it behind the stream).
 *   workspace: gsv_sola_workspace(search_len) bytes, device.  Two launches, nothing allocated. */
size_t gsv_sola_workspace(int search_len);
int gsv_sola(const float* prev_tail, const float* chunk, int n, int overlap, int search_len, float* out, int32_t* offset,
             void* workspace, size_t workspace_bytes, void* stream);

/* Chunk epilogue of a stream: everything TTS.infer_stream does between the decode of a chunk and its hand-out (TTS.py:429-470: the
 * splice above, the tail kept back, the head trim of TTS._find_head_threshold_offsets on a segment's first chunk, the mute behind its
 * last), in that order, with no value read by the host in between -- many streams can be served from one loop.
 *   prev_tail fp32 [overlap] or NULL (first chunk of a segment: offset 0, no cross-fade); chunk fp32 [n], n >= overlap.
 *   k: gsv_sola's offset; s: gsv_sola's spliced signal, m = n - k samples, bit for bit.
 *   tail_out fp32 [overlap] = s[m - overlap : m]; it must not alias prev_tail (keep two tails and use them in turn).
 *   body = s if is_final, else s[: m - overlap].
 *   h = 0 unless trim_head: over the first L = min(len(body), 64000) samples of body, in frames of 512 with hop 256, the first
 *   frame f with sqrtf(sum of squares / 512) > 0.02f gives h = max(0, 256 f - 3200); no such frame, or L < 512: h = L.  The fp32 sum
 *   of a frame is H[f] + H[f + 1]; H[j], over the 256 samples from 256 j, is taken by 64 lanes: lane l adds s[256 j + l + 64 t]^2 for
 *   t = 0..3 in that order (fused multiply-add), then the lanes are added pairwise at strides 32, 16, 8, 4, 2, 1.
 *   -> out fp32 (capacity n + mute_samples) = body[h:], followed by mute_samples zeros if is_final;
 *      rec int32 [4] (device) = {samples written to out, k, h, 0}: copy it with `out` behind the stream.
 *   workspace: gsv_stream_emit_workspace(search_len, n) bytes, device (0: a negative argument).  Three launches (score -- with a tail
 *   only --, decide, copy), nothing allocated, nothing read by the host.  GSV_ERR_ARG: n < overlap, a negative size, overlap < 1 with a
 *   tail, tail_out == prev_tail, or a workspace that is too small. */
size_t gsv_stream_emit_workspace(int search_len, int n);
int gsv_stream_emit(const float* prev_tail, const float* chunk, int n, int overlap, int search_len, int is_final, int trim_head,
                    int mute_samples, float* out, float* tail_out, int32_t* rec, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Real-time track output: a stream of fp32 samples at in_rate -> s16 packets of `packet` samples per channel at out_rate,
 * whatever the chunks the stream arrives in (csrc/track.h).  With the rates reduced by their gcd to o and w,
 * width and L = 2 width + o as gsv_sv_resample has them and K torchaudio's sinc table (built on the HOST in fp64, cast to
 * fp32 and uploaded, so device and host twin share its bits), a stream x[0, N) gives M = ceil(w N / o) outputs
 *   y[j w + p] = sum_{i < L} x[j o - width + i] K[p][i]   (samples outside [0, N) skipped; fp32, tap order, fused multiply-add),
 * y = x if o == w; q = the FLAC writer's quantiser at 16 bits (x 2^15, round half to even, clamp, NaN -> 0); with 2 channels
 * every q is written twice, interleaved; the s16 stream is cut into packets, and a flush fills the last with zeros.
 * After N_t samples the outputs that exist are the first min(w J, ceil(w N_t / o)), J = 0 if N_t < width + o, else
 * (N_t - width - o) / o + 1 (N_t if o == w); a flush makes the rest up to M and returns the state to fresh.
 *   state: caller-owned, gsv_track_state_bytes bytes (0: bad arguments -- packet 1..4096, channels 1 or 2, a rate pair
 *   gsv_sv_resample accepts), 16-byte aligned, made by gsv_track_init: a header (samples in, outputs out, samples carried), the
 *   table, a ring of the last L + o input samples, a carry of packet x channels int16.
 *   gsv_track_out_capacity: the int16 elements a push of at most n_cap samples can write (what `out` must hold).
 *   gsv_track_push: chunk fp32 [n_cap] (may be NULL when n_cap is 0); n_dev NULL or a device int32 holding the real length
 *   (clamped to 0..n_cap) -- gsv_stream_emit's rec, so the call sits directly behind it --; out: whole packets, contiguous
 *   (the samples of the next, partial packet lie behind them until the second launch has moved them to the carry);
 *   rec int32 [4] (device) = {packets written, outputs produced by this call, samples per channel left in the carry, zeros
 *   per channel padded by the flush}.  Two launches, nothing allocated, nothing read by the host.
 *   gsv_track_init_host / gsv_track_push_host: the same over HOST memory from the same scalar routines -- the CPU path and
 *   the device's oracle (device bytes equal host bytes); they need no GPU.
 * GSV_ERR_ARG: a null pointer, a negative size, bad rates / packet / channels, a state that is too small or misaligned. */
size_t gsv_track_state_bytes(int in_rate, int out_rate, int packet, int channels);
size_t gsv_track_out_capacity(int n_cap, int in_rate, int out_rate, int packet, int channels);
int gsv_track_init(void* state, size_t bytes, int in_rate, int out_rate, int packet, int channels, void* stream);
int gsv_track_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, int16_t* out, int32_t* rec,
                   void* stream);
int gsv_track_init_host(void* state, size_t bytes, int in_rate, int out_rate, int packet, int channels);
int gsv_track_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, int16_t* out,
                        int32_t* rec);

/* Loudness: ITU-R BS.1770 integrated loudness (K-weighting, 400 ms blocks overlapping by 75 %, the absolute gate at -70 LUFS
 * and the relative gate 10 LU under it) of n_clips clips of one packed fp32 buffer, and each clip scaled to its target
 * (csrc/loudness.h).  The meter is the one pyloudnorm implements (its shelf design included), in fp64.
 *   x: fp32 [n_x]; clip c is x[offset, offset + n_samples), mono at `rate` Hz (4000..768000); the clips do not overlap.
 *   target: LUFS, NaN for a clip that is only measured.  peak_limit > 0: no gain lifts a clip's peak above it (inf: no limit).
 *   out: NULL (measure only), x (in place) or a second buffer of n_x floats; only [offset, offset + n_samples) of each clip
 *   is written: x * gain, one fp32 product (a gain of 1 copies the samples, and writes nothing in place).
 *   records [n_clips]: zbar the mean square of the blocks past both gates -- the loudness is -0.691 + 10 log10(zbar) LUFS --,
 *   the gain applied = min(sqrt(10^((target + 0.691) / 10) / zbar), peak_limit / peak) rounded to fp32 -- and, when the limit is
 *   the smaller one and the fp32 product gain * peak would still round above peak_limit, one ulp less --, the input peak max|x|, the blocks,
 *   those at or above the absolute gate, those past both gates, and flags.  A clip shorter than one block, a clip with no
 *   block past the gates and a clip holding a NaN or an infinity (GSV_LOUD_NONFINITE) have no measurement: zbar 0, gain 1,
 *   GSV_LOUD_MEASURED clear, samples unchanged.  The filtered signal is held as fp32, saturating: a finite sample so close to
 *   FLT_MAX that the shelf lifts it past the fp32 range is measured at FLT_MAX (zbar and the gain stay finite).
 *   work: caller-owned, gsv_loudness_work_bytes(clips, n_clips, rate) bytes (0: bad arguments), 16-byte aligned.
 *   gsv_loudness: x, out, records and work are DEVICE memory, clips is HOST memory.  One small upload and at most seven launches
 *   on `stream` (a clip longer than 16 384 samples is filtered in chunks side by side, their states chained); nothing allocated, nothing read back by the host.
 *   gsv_loudness_host: the same over HOST memory from the same scalar routines -- the CPU path and the device's oracle
 *   (device records and samples equal the host's bit for bit); it needs no GPU.
 * GSV_ERR_ARG: a null pointer, a bad rate / peak_limit / clip count (1..65535), a clip outside [0, n_x), a workspace that
 * is too small or misaligned. */
typedef struct {
    int64_t offset;         /* first sample of the clip in x */
    int32_t n_samples;
    float target;           /* LUFS; NaN: measure only */
} gsv_loudness_clip;
typedef struct {
    double zbar;
    float gain;
    float peak;
    int32_t blocks, above_abs, kept, flags;
} gsv_loudness_record;
#define GSV_LOUD_LIMITED 1      /* the peak limit was the smaller gain */
#define GSV_LOUD_MEASURED 2
#define GSV_LOUD_NONFINITE 4    /* a NaN or an infinity among the samples */
size_t gsv_loudness_work_bytes(const gsv_loudness_clip* clips, int n_clips, int rate);
int gsv_loudness(const float* x, size_t n_x, const gsv_loudness_clip* clips, int n_clips, int rate, float peak_limit, float* out,
                 gsv_loudness_record* records, void* work, size_t work_bytes, void* stream);
int gsv_loudness_host(const float* x, size_t n_x, const gsv_loudness_clip* clips, int n_clips, int rate, float peak_limit,
                      float* out, gsv_loudness_record* records, void* work, size_t work_bytes);

/* Stream leveller: a running BS.1770 gain for a stream of fp32 samples, whatever the chunks it arrives in (csrc/level.h,
 * DESIGN 4.21).  Sample indices count from the start of the stream; knot h is l_h = (int)(0.4 * (h * 0.25) * rate), hop h is
 * [l_h, l_(h+1)), block j is hops j .. j + 3.  The K-filter of gsv_loudness runs over the stream from zero state, complete hops
 * only; S_h is a hop's sum of y^2, z_j = (S_j + S_(j+1) + S_(j+2) + S_(j+3)) / (0.4 rate); after hops < h both gates of
 * gsv_loudness over blocks 0 .. h - 4 give kept_h and zbar_h, and P_h is the largest |x| of those hops.  The gain at knot h + 1:
 *   z_eff = (w seed_z + kept_h zbar_h) / (w + kept_h), seed_z = 10^((seed_lufs + 0.691) / 10), w = seed_blocks (no seed: w = 0);
 *   d = sqrt(10^((target + 0.691) / 10) / z_eff) (1 when w + kept_h is 0), clamped to [1 / G, G], G = 10^(max_gain_db / 20),
 *   then to at most peak_limit / P_h;  A_(h+1) = min(max(d, A_h / r), A_h r), r = 10^(slew_db_s * 0.1 / 20);
 *   A_0 = the seed's gain clamped to [1 / G, G], or 1.
 * A sample n of hop h gets a = (float)fma(A_(h+1) - A_h, (double)(n - l_h) / (double)(l_(h+1) - l_h), A_h); y = x * a is one
 * fp32 product; |y| > peak_limit becomes +-peak_limit and is counted.  Every decision is fp64; the knot a sample needs is
 * decided from hops that ended before the sample's hop began, so the leveller adds no delay.
 * A hop holding a NaN or an infinity is not measured and freezes the measure (GSV_LEVEL_NONFINITE): the last knot's gain holds.
 * So does a full block history (GSV_LEVEL_FULL): max_seconds (1..3600) sizes it, (max_seconds - 0.4) / 0.1 + 1 blocks.
 *   state: caller-owned, gsv_level_state_bytes(rate, max_seconds) bytes (0: a rate outside 4000..192000 or a bad max_seconds),
 *   16-byte aligned, made by gsv_level_init: a header with every constant, the knots, the hop sums, the blocks, and a ring of
 *   the newest samples in which an incomplete hop waits.  After N samples of the first stream
 *   on a state as gsv_level_init left it, it is the same byte for byte however they were pushed (a flush marks the state ended
 *   and leaves the old stream's arrays where the next has not overwritten them: unread, but there).
 *   seed_lufs: NaN for no seed.  peak_limit > 0 (inf: no limit).
 *   gsv_level_push: chunk fp32 [n_cap] (may be NULL when n_cap is 0); n_dev NULL or a device int32 holding the real length
 *   (clamped to 0..n_cap) -- gsv_stream_emit's rec, so the call sits directly behind it --; out fp32 [n_cap], may be chunk;
 *   flush ends the stream: the incomplete hop has been output and is never measured, and the next push starts a fresh stream
 *   with the same constants.  rec (device, 8-byte aligned): the running measure of the UNLEVELLED stream after this push, the
 *   gain of the push's first and last sample (an empty push: of the next sample), the samples clamped so far, the blocks,
 *   those at or above the absolute gate, those past both gates, and flags.  A state gsv_level_init did not make is not read
 *   through: the record says flags -1 and `out` is not written.  Two launches, nothing allocated, nothing read by the host.
 *   gsv_level_init_host / gsv_level_push_host: the same over HOST memory from the same scalar routines -- the CPU path and
 *   the device's oracle (device samples, records and state bytes equal the host's); they need no GPU.
 * GSV_ERR_ARG: a null pointer, a negative size, a bad rate / max_seconds / constant, a state that is too small or misaligned,
 * a misaligned record. */
typedef struct {
    double zbar;
    float gain_first, gain_last;
    int64_t clamped;
    int32_t blocks, above_abs, kept, flags;
} gsv_level_record;
#define GSV_LEVEL_MEASURED 2
#define GSV_LEVEL_NONFINITE 4   /* a NaN or an infinity in a hop: the measure is frozen */
#define GSV_LEVEL_FULL 8        /* the block history is full: the measure is frozen */
size_t gsv_level_state_bytes(int rate, int max_seconds);
int gsv_level_init(void* state, size_t bytes, int rate, double target, double seed_lufs, double seed_blocks, double slew_db_s,
                   double max_gain_db, float peak_limit, int max_seconds, void* stream);
int gsv_level_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out, gsv_level_record* rec,
                   void* stream);
int gsv_level_init_host(void* state, size_t bytes, int rate, double target, double seed_lufs, double seed_blocks,
                        double slew_db_s, double max_gain_db, float peak_limit, int max_seconds);
int gsv_level_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                        gsv_level_record* rec);

/* True-peak limiter: the true peak of n_clips clips of one packed fp32 buffer, and each clip held under its ceiling by a
 * look-ahead limiter (csrc/limiter.h).  With T = 10^(ceiling_db / 20), L = lookahead and s = 1 / release:
 *   e[n] = max |u[4n-3 .. 4n+3]|, u the clip oversampled 4x by the 49-tap sinc(k/4) kaiser(49, 8) (12 taps per phase, phase 0
 *   the identity, zeros outside the clip); c = min(1, T / e); h[n] = min c[n .. n+L-1] (c = 1 behind the end);
 *   r[n] = min(h[n], min_{k<=n}(h[k] + (n-k) s)); g[n] = min(c[n], (sum_{i<L} r[n-i]) (1/L)) with r[m<0] = r[0]; y1 = g x;
 *   t = min(1, T / truepeak(y1)); y = t y1.  All fp32.
 *   x: fp32 [n_x]; clip c is x[offset, offset + n_samples), mono; the clips do not overlap.  ceiling_db: dBTP in -200..0, NaN
 *   for a clip that is only measured.  lookahead 1..4096 and release 1..2^24 are in samples.
 *   out: NULL (measure only), x (in place) or a second buffer of n_x floats; only [offset, offset + n_samples) of each clip
 *   is written.  A clip whose true peak is at or under its ceiling is copied (in place: nothing is written).
 *   records [n_clips]: true_peak_in = max e; true_peak_out = trim * truepeak(y1) (true_peak_in for a clip that was not
 *   limited); min_gain = min g and trim = t (both 1 for such a clip); flags; the look-ahead and the release of the call.  A
 *   clip holding a NaN or an infinity (GSV_LIM_NONFINITE) comes back unchanged, its peaks that NaN or infinity.
 *   work: caller-owned, gsv_limiter_work_bytes(clips, n_clips) bytes (0: bad arguments), 16-byte aligned.
 *   gsv_limiter: x, out, records and work are DEVICE memory, clips is HOST memory.  One small upload and at most six launches
 *   on `stream`; nothing allocated, nothing read back by the host.
 *   gsv_limiter_host: the same over HOST memory from the same scalar routines -- the CPU path and the device's oracle
 *   (device records and samples equal the host's bit for bit); it needs no GPU.
 * GSV_ERR_ARG: a null pointer, a bad look-ahead / release / ceiling / clip count (1..65535), a clip outside [0, n_x), a
 * workspace that is too small or misaligned. */
typedef struct {
    int64_t offset;         /* first sample of the clip in x */
    int32_t n_samples;
    float ceiling_db;       /* dBTP; NaN: measure only */
} gsv_limiter_clip;
typedef struct {
    float true_peak_in, true_peak_out, min_gain, trim;
    int32_t flags, lookahead, release, reserved;
} gsv_limiter_record;
#define GSV_LIM_LIMITED 1       /* the true peak was above the ceiling: the clip was limited */
#define GSV_LIM_NONFINITE 4     /* a NaN or an infinity among the samples */
size_t gsv_limiter_work_bytes(const gsv_limiter_clip* clips, int n_clips);
int gsv_limiter(const float* x, size_t n_x, const gsv_limiter_clip* clips, int n_clips, int lookahead, int release, float* out,
                gsv_limiter_record* records, void* work, size_t work_bytes, void* stream);
int gsv_limiter_host(const float* x, size_t n_x, const gsv_limiter_clip* clips, int n_clips, int lookahead, int release,
                     float* out, gsv_limiter_record* records, void* work, size_t work_bytes);

/* Stream limiter: the limiter above for a stream that arrives in pushes (csrc/limstream.h).  The output is
 * stages e .. y1 of gsv_limiter applied to the whole stream as one clip, y[n] = g[n] x[n], with three differences: no trim; no
 * "a clip under its ceiling is not touched"; instead a window whose L values of r are all exactly 1 gives g = 1 and the sample
 * is copied.  y[n] is final once x[n + L + 5] has arrived: the limiter delays the stream by D = lookahead + 5 samples.  After N
 * samples max(0, N - D) outputs have been emitted (a push may emit none); a flush emits the rest (zeros behind the end of x,
 * c = 1 behind the end) and returns the state to fresh.  The emitted bytes never depend on how the stream was cut into pushes:
 * the release is computed on 1024-sample tiles aligned to the stream index with the clip kernels' operations, and a tile a
 * push leaves unfinished is redone from its h, so for a stream that is limited somewhere the output equals fl(g x) with g the
 * stage array of gsv_limiter for the same samples as one clip, bit for bit (at a look-ahead with fl(L fl(1/L)) == 1).  A sample
 * whose envelope is not finite needs gain 1 and is copied (GSV_LIMS_NONFINITE); such envelopes are kept out of the peaks.
 * |y[n]| <= T (1 + 2^-22); the TRUE peak of y may exceed T by what the gain smoothing moves peaks between the samples.
 *   state: caller-owned, gsv_limstream_state_bytes bytes (0: lookahead outside 1..4096 or release outside 1..2^24), 16-byte
 *   aligned, made by gsv_limstream_init: a header, the constants, a ring of the newest lookahead + 11 samples, h of the open
 *   tile, r of the last lookahead - 1 outputs, the chain's start, and the per-push scratch of the tile ends.
 *   gsv_limstream_out_capacity: n_cap + D, the floats `out` must hold (0: bad arguments).
 *   gsv_limstream_push: chunk fp32 [n_cap], n_cap 0..2^20 (NULL allowed at 0); n_dev NULL or a device int32 holding the real
 *   length (clamped to 0..n_cap); out != chunk; rec (device, 8-byte aligned).  Three launches whatever the length, nothing
 *   allocated, nothing read by the host.  A state gsv_limstream_init did not make is not read through: flags -1.
 *   gsv_limstream_init_host / gsv_limstream_push_host: the same over HOST memory from the same scalar routines -- the CPU path
 *   and the device's oracle (device samples and records equal the host's); they need no GPU.
 * GSV_ERR_ARG: a null pointer, a size that is negative or above 2^20, out == chunk, a state that is too small or misaligned, a
 * misaligned record, a ceiling outside -200..0 dBTP, a bad look-ahead / release. */
typedef struct {
    int32_t emitted;            /* samples this push wrote to out: its address serves as the next stage's n_dev */
    int16_t flags, lookahead;
    float peak_in;              /* max finite e over the samples emitted by this push (0: none) */
    float peak_run;             /* ... by the stream so far */
    float min_gain;             /* min g over the samples emitted by this push (1: none) */
    int32_t release;
    int64_t total;              /* samples emitted by the stream so far */
} gsv_limstream_record;
#define GSV_LIMS_LIMITED 1          /* a gain below 1 among this push's samples */
#define GSV_LIMS_LIMITED_EVER 2     /* ... among the stream's so far */
#define GSV_LIMS_NONFINITE 4        /* an envelope that is not finite among this push's samples */
size_t gsv_limstream_state_bytes(int lookahead, int release);
size_t gsv_limstream_out_capacity(int n_cap, int lookahead);
int gsv_limstream_init(void* state, size_t bytes, float ceiling_db, int lookahead, int release, void* stream);
int gsv_limstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out,
                       gsv_limstream_record* rec, void* stream);
int gsv_limstream_init_host(void* state, size_t bytes, float ceiling_db, int lookahead, int release);
int gsv_limstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                            gsv_limstream_record* rec);

/* Equaliser: n_clips clips of one packed fp32 buffer, each through one of n_designs cascades of 1 to 6 second-order sections
 * (csrc/eq.h).  Per section, in list order, from zero state, in fp64 (transposed direct form II):
 *   y = b0 x + z0;  z0 = b1 x - a1 y + z1;  z1 = b2 x - a2 y;
 * fp64 between the sections; the last section's output is rounded once to fp32, saturating at +-FLT_MAX.  Same length out as in.
 *   designs [n_designs] (HOST memory in both entries): per section b0 b1 b2 a1 a2, normalised by a0.  Whoever designs the
 *   sections needs the sampling rate; this call does not.
 *   x: fp32 [n_x]; clip c is x[offset, offset + n_samples), mono; the clips do not overlap.  design: an index into designs,
 *   or -1 for a clip whose peaks are measured and whose samples are copied.
 *   out: x (in place) or a second buffer of n_x floats; only [offset, offset + n_samples) of each clip is written.
 *   records [n_clips]: peak_in = max |x|, peak_out = max |y| (nothing clamps y: boosts may lift it above 1), the sections run
 *   and flags.  A clip holding a NaN or an infinity (GSV_EQ_NONFINITE) comes back bit for bit, sections 0, peak_out = peak_in
 *   = that NaN or infinity; so does a clip with design -1, flags 0.  An empty clip is legal.
 *   work: caller-owned, gsv_eq_work_bytes(clips, n_clips, designs, n_designs) bytes (0: bad arguments), 16-byte aligned.
 *   gsv_eq: x, out, records and work are DEVICE memory, clips and designs HOST memory.  One small upload (the clip rows, the
 *   coefficients, the scan's matrices) and at most four launches on `stream`; nothing allocated, nothing read back by the host.
 *   gsv_eq_host: the same over HOST memory from the same scalar routines -- the CPU path and the device's oracle (device
 *   records and samples equal the host's bit for bit); it needs no GPU.
 * GSV_ERR_ARG: a null pointer, a bad clip or design count (1..65535 clips, 0..65535 designs), a design index outside the
 * designs, a clip outside [0, n_x), a section count outside 1..6, a coefficient that is not finite, a section whose poles are
 * not inside the unit circle (it needs |a2| < 1 and |a1| < 1 + a2), a workspace that is too small or misaligned. */
#define GSV_EQ_MAX_SECTIONS 6
typedef struct {
    int64_t offset;         /* first sample of the clip in x */
    int32_t n_samples;
    int32_t design;         /* index into designs; -1: measure the peaks, copy */
} gsv_eq_clip;
typedef struct {
    int32_t n_sections, reserved;
    double coef[GSV_EQ_MAX_SECTIONS][5];    /* b0 b1 b2 a1 a2 */
} gsv_eq_design;
typedef struct {
    float peak_in, peak_out;
    int32_t sections, flags;
} gsv_eq_record;
#define GSV_EQ_EQUALISED 1      /* the sections were run over the clip */
#define GSV_EQ_NONFINITE 4      /* a NaN or an infinity among the samples */
size_t gsv_eq_work_bytes(const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs);
int gsv_eq(const float* x, size_t n_x, const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs,
           float* out, gsv_eq_record* records, void* work, size_t work_bytes, void* stream);
int gsv_eq_host(const float* x, size_t n_x, const gsv_eq_clip* clips, int n_clips, const gsv_eq_design* designs, int n_designs,
                float* out, gsv_eq_record* records, void* work, size_t work_bytes);

/* Compressor: n_clips clips of one packed fp32 buffer, each through a feed-forward compressor with one of n_params parameter
 * sets (csrc/compressor.h).  The level detector is the smooth decoupled peak detector (Giannoulis, Massberg, Reiss,
 * JAES 2012), from zero state, in fp64, with a hard knee:
 *   p = max(|x|, release p + (1 - release) |x|);  e = attack e + (1 - attack) p;
 *   g = e <= threshold ? 1 : exp2(slope log2(e / threshold));  y = fp32(makeup g x), saturating at +-FLT_MAX.
 *   params [n_params] (HOST memory in both entries): attack and release are the one-pole coefficients exp(-2 pi 1000 / (rate ms))
 *   in (0, 1), threshold and makeup linear and positive, slope = 1 / ratio - 1 in [-1, 0].  Whoever makes them needs the sampling
 *   rate; this call does not.
 *   x: fp32 [n_x]; clip c is x[offset, offset + n_samples), mono; the clips do not overlap.  params: an index into params, or -1
 *   for a clip whose peaks are measured and whose samples are copied.
 *   out: x (in place) or a second buffer of n_x floats; only [offset, offset + n_samples) of each clip is written.
 *   records [n_clips]: peak_in = max |x|, peak_out = max |y|, min_gain = the smallest g as fp32 (makeup excluded) and flags:
 *   GSV_CMP_COMPRESSED when min_gain < 1.  A clip that never passes its threshold, with makeup 1, comes back bit for bit.  A clip
 *   holding a NaN or an infinity (GSV_CMP_NONFINITE) comes back bit for bit, min_gain 1, peak_out = peak_in = that NaN or
 *   infinity; so does a clip with params -1, flags 0.  An empty clip is legal.
 *   work: caller-owned, gsv_compressor_work_bytes(clips, n_clips, params, n_params) bytes (0: bad arguments), 16-byte aligned.
 *   gsv_compressor: x, out, records and work are DEVICE memory, clips and params HOST memory.  One small upload (the clip rows,
 *   the parameters, the scans' powers) and at most six launches on `stream`; nothing allocated, nothing read back by the host.
 *   gsv_compressor_host: the same over HOST memory from the same scalar routines -- the CPU path and the device's oracle (device
 *   records and samples equal the host's bit for bit); it needs no GPU.
 *   gsv_compressor_math_host: out[i] = the call's own log2 (which 0; positive normal arguments) or exp2 (which 1; the argument
 *   clamped to [-1000, 1000]) of in[i], on the host: what the kernels evaluate, for whoever wants to measure it.
 * GSV_ERR_ARG: a null pointer, a bad clip or parameter-set count (1..65535 clips, 0..65535 sets), an index outside the sets, a
 * clip outside [0, n_x), a parameter outside the ranges above, a workspace that is too small or misaligned. */
typedef struct {
    int64_t offset;         /* first sample of the clip in x */
    int32_t n_samples;
    int32_t params;         /* index into params; -1: measure the peaks, copy */
} gsv_compressor_clip;
typedef struct {
    double attack, release; /* one-pole coefficients, in (0, 1) */
    double threshold;       /* linear, > 0 */
    double slope;           /* 1 / ratio - 1, in [-1, 0] */
    double makeup;          /* linear, > 0 */
} gsv_compressor_params;
typedef struct {
    float peak_in, peak_out;
    float min_gain;
    int32_t flags;
} gsv_compressor_record;
#define GSV_CMP_COMPRESSED 1    /* the gain went below 1 somewhere in the clip */
#define GSV_CMP_NONFINITE 4     /* a NaN or an infinity among the samples */
size_t gsv_compressor_work_bytes(const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params, int n_params);
int gsv_compressor(const float* x, size_t n_x, const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params,
                   int n_params, float* out, gsv_compressor_record* records, void* work, size_t work_bytes, void* stream);
int gsv_compressor_host(const float* x, size_t n_x, const gsv_compressor_clip* clips, int n_clips, const gsv_compressor_params* params,
                        int n_params, float* out, gsv_compressor_record* records, void* work, size_t work_bytes);
int gsv_compressor_math_host(int which, const double* in, double* out, size_t n);

/* Reverb: n_clips clips of one packed fp32 buffer, each through Freeverb -- eight parallel damped comb filters, their sum through
 * four all-pass filters in series -- with one of n_params parameter sets (csrc/reverb.h).  From zero state, in fp64,
 * per sample, v = x[n]:
 *   u = gin v;   comb k: o_k = b_k[n - comb[k]];  l_k = (1 - d) o_k + d l_k;  b_k[n] = u + fb l_k;
 *   s = ((((((o_0 + o_1) + o_2) + o_3) + o_4) + o_5) + o_6) + o_7;
 *   all-pass j in order: t = a_j[n - allpass[j]];  a_j[n] = s + 0.5 t;  s = t - s;
 *   y = fp32(gw s + gd v), saturating at +-FLT_MAX.  The output has the clip's length: the tail behind it is cut.
 *   params [n_params] (HOST memory in both entries): the twelve delays in samples, each 1..GSV_RVB_MAX_DELAY; d and fb in [0, 1);
 *   gin, gw, gd finite.  Whoever makes them needs the sampling rate; this call does not.
 *   x: fp32 [n_x]; clip c is x[offset, offset + n_samples), mono; the clips do not overlap.  params: an index into params, or -1
 *   for a clip whose peaks are measured and whose samples are copied.
 *   out: x (in place) or a second buffer of n_x floats; only [offset, offset + n_samples) of each clip is written.
 *   records [n_clips]: peak_in = max |x|, peak_out = max |y| and flags: GSV_RVB_REVERBED for a clip that went through the network.
 *   A clip holding a NaN or an infinity (GSV_RVB_NONFINITE) comes back bit for bit, peak_out = peak_in = that NaN or infinity; so
 *   does a clip with params -1, flags 0.  An empty clip is legal.
 *   work: caller-owned, gsv_reverb_work_bytes(clips, n_clips, params, n_params) bytes (0: bad arguments), 16-byte aligned; 72
 *   bytes per sample of the clips that have a parameter set.
 *   gsv_reverb: x, out, records and work are DEVICE memory, clips and params HOST memory.  One small upload (the clip rows, the
 *   parameters, the scan's powers) and seven launches on `stream`; nothing allocated, nothing read back by the host.
 *   gsv_reverb_host: the same over HOST memory from the same scalar routines -- the CPU path and the device's oracle (device
 *   records and samples equal the host's bit for bit); it needs no GPU.
 * GSV_ERR_ARG: a null pointer, a bad clip or parameter-set count (1..65535 clips, 0..65535 sets), an index outside the sets, a
 * clip outside [0, n_x), a delay, d, fb or a gain outside the ranges above, a workspace that is too small or misaligned. */
typedef struct {
    int64_t offset;         /* first sample of the clip in x */
    int32_t n_samples;
    int32_t params;         /* index into params; -1: measure the peaks, copy */
} gsv_reverb_clip;
typedef struct {
    int32_t comb[8];        /* the comb delays in samples, each 1..GSV_RVB_MAX_DELAY */
    int32_t allpass[4];     /* the all-pass delays in samples, likewise */
    double d, fb;           /* damping and feedback, each in [0, 1) */
    double gin, gw, gd;     /* input, wet and dry gains, finite */
} gsv_reverb_params;
typedef struct {
    float peak_in, peak_out;
    int32_t flags, pad;
} gsv_reverb_record;
#define GSV_RVB_REVERBED 1      /* the clip went through the network */
#define GSV_RVB_NONFINITE 4     /* a NaN or an infinity among the samples */
#define GSV_RVB_MAX_DELAY 32768
size_t gsv_reverb_work_bytes(const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params);
int gsv_reverb(const float* x, size_t n_x, const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params,
               float* out, gsv_reverb_record* records, void* work, size_t work_bytes, void* stream);
int gsv_reverb_host(const float* x, size_t n_x, const gsv_reverb_clip* clips, int n_clips, const gsv_reverb_params* params, int n_params,
                    float* out, gsv_reverb_record* records, void* work, size_t work_bytes);

/* Stream equaliser: the equaliser above for a stream that arrives in pushes (csrc/eqstream.h).  An equaliser is
 * causal: a push of n samples emits n samples (no delay), a flush emits nothing extra (no ring-out) and returns the state to
 * fresh, so that the next push starts a new stream with the same design.  The emitted samples, concatenated, are the bytes
 * gsv_eq / gsv_eq_host return for the same finite samples as one clip with the same design, however the stream was cut into
 * pushes: the stream runs the clip kernels' operations on 16384-sample chunks aligned to the stream index, and a chunk a push
 * leaves unfinished is redone from its start state over its kept input.  A sample that is not finite enters the filter as 0.0
 * and is copied to the output bit for bit (GSV_EQS_NONFINITE on the push, GSV_EQS_NONFINITE_EVER on the stream); it is kept out
 * of the peaks, and every other output equals the stream with that sample replaced by 0.0.  Nothing clamps y.
 *   state: caller-owned, gsv_eqstream_state_bytes() bytes, 16-byte aligned, made by gsv_eqstream_init from one design (HOST
 *   memory in both entries): a header, the open chunk's joint start state, the coefficients and the scan's matrices, the open
 *   chunk's input so far in two copies used in turn, and the per-push scratch of the chunk states.
 *   gsv_eqstream_push: chunk fp32 [n_cap], n_cap 0..2^20 (chunk and out may be NULL at 0); n_dev NULL or a device int32 holding
 *   the real length (clamped to 0..n_cap), e.g. gsv_stream_emit's record; out fp32 [n_cap], which may be chunk (in place): the
 *   first `emitted` are written, nothing behind them; rec (device, 8-byte aligned).  Four launches whatever the length (two at
 *   n_cap 0), nothing allocated, nothing read by the host.  A state gsv_eqstream_init did not make is not read through: flags
 *   -1, out not written.
 *   gsv_eqstream_init_host / gsv_eqstream_push_host: the same over HOST memory from the same scalar routines -- the CPU path
 *   and the device's oracle (device samples and records equal the host's bit for bit); they need no GPU.
 * GSV_ERR_ARG: a null pointer, a size that is negative or above 2^20, a design gsv_eq would refuse, a state that is too small or
 * misaligned, a misaligned record. */
typedef struct {
    int32_t emitted;            /* samples this push wrote to out: its address serves as the next stage's n_dev */
    int32_t flags;
    float peak_in, peak_out;    /* max |x|, max |y| over the finite samples of this push (0: none) */
    float peak_in_run, peak_out_run;    /* ... of the stream so far */
    int64_t total;              /* samples of the stream so far (a flush reports the stream's length) */
} gsv_eqstream_record;
#define GSV_EQS_EQUALISED 1         /* the record of a state gsv_eqstream_init made */
#define GSV_EQS_NONFINITE_EVER 2    /* a NaN or an infinity among the stream's samples so far */
#define GSV_EQS_NONFINITE 4         /* ... among this push's samples */
size_t gsv_eqstream_state_bytes(void);
int gsv_eqstream_init(void* state, size_t bytes, const gsv_eq_design* design, void* stream);
int gsv_eqstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out,
                      gsv_eqstream_record* rec, void* stream);
int gsv_eqstream_init_host(void* state, size_t bytes, const gsv_eq_design* design);
int gsv_eqstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                           gsv_eqstream_record* rec);

/* Stream compressor: the compressor above for a stream that arrives in pushes (csrc/cmpstream.h).  The compressor
 * is causal: a push of n samples emits n samples (no delay), a flush emits nothing extra (no ring-out) and returns the state to
 * fresh, so that the next push starts a new stream with the same parameters.  The emitted samples, concatenated, are the bytes
 * gsv_compressor / gsv_compressor_host return for the same finite samples as one clip with the same parameters, however the
 * stream was cut into pushes: the stream runs the clip kernels' three passes and two chains on 16384-sample chunks aligned to
 * the stream index, and a chunk a push leaves unfinished is redone from its start states over its kept input.  A sample that is
 * not finite enters the detector as 0.0 and is copied to the output bit for bit (GSV_CMS_NONFINITE on the push,
 * GSV_CMS_NONFINITE_EVER on the stream); it is kept out of the peaks and of the smallest gain, and every other output equals the
 * stream with that sample replaced by 0.0.
 *   state: caller-owned, gsv_cmpstream_state_bytes() bytes, 16-byte aligned, made by gsv_cmpstream_init from one parameter set
 *   (HOST memory in both entries): a header, the coefficients and their powers, the open chunk's start states of the release and
 *   the attack, the open chunk's input so far in two copies used in turn, and the per-push scratch of the chunk states.
 *   gsv_cmpstream_push: chunk fp32 [n_cap], n_cap 0..2^20 (chunk and out may be NULL at 0); n_dev NULL or a device int32 holding
 *   the real length (clamped to 0..n_cap), e.g. gsv_stream_emit's or gsv_eqstream_push's record; out fp32 [n_cap], which may be
 *   chunk (in place): the first `emitted` are written, nothing behind them; rec (device, 8-byte aligned).  Six launches whatever
 *   the length (three at n_cap 0), nothing allocated, nothing read by the host.  A state gsv_cmpstream_init did not make is not
 *   read through: flags -1, out not written.
 *   gsv_cmpstream_init_host / gsv_cmpstream_push_host: the same over HOST memory from the same scalar routines -- the CPU path
 *   and the device's oracle (device samples and records equal the host's bit for bit); they need no GPU.
 * GSV_ERR_ARG: a null pointer, a size that is negative or above 2^20, parameters gsv_compressor would refuse, a state that is too
 * small or misaligned, a misaligned record. */
typedef struct {
    int32_t emitted;            /* samples this push wrote to out: its address serves as the next stage's n_dev */
    int32_t flags;
    float peak_in, peak_out;    /* max |x|, max |y| over the finite samples of this push (0: none) */
    float min_gain;             /* the smallest gain (makeup excluded) among them (1: none) */
    float peak_in_run, peak_out_run, min_gain_run;      /* ... of the stream so far */
    int64_t total;              /* samples of the stream so far (a flush reports the stream's length) */
} gsv_cmpstream_record;
#define GSV_CMS_STREAM 1            /* the record of a state gsv_cmpstream_init made */
#define GSV_CMS_NONFINITE_EVER 2    /* a NaN or an infinity among the stream's samples so far */
#define GSV_CMS_NONFINITE 4         /* ... among this push's samples */
#define GSV_CMS_COMPRESSED 8        /* min_gain < 1: the compressor acted on this push */
size_t gsv_cmpstream_state_bytes(void);
int gsv_cmpstream_init(void* state, size_t bytes, const gsv_compressor_params* params, void* stream);
int gsv_cmpstream_push(void* state, const float* chunk, int n_cap, const int32_t* n_dev, int flush, float* out,
                       gsv_cmpstream_record* rec, void* stream);
int gsv_cmpstream_init_host(void* state, size_t bytes, const gsv_compressor_params* params);
int gsv_cmpstream_push_host(void* state, const float* chunk, int n_cap, const int32_t* n_host, int flush, float* out,
                            gsv_cmpstream_record* rec);

/* Reference-audio path, once per new speaker / prompt; fp32 in both numerics modes.
 * Replaces, on the device:
 *   gsv_ref_spectrogram     the torchaudio Spectrogram inside TTS._get_spec (gsv_tts/TTS.py:1591-1604: n_fft /
 *                           win = filter_length, hop_length, periodic hann, center + reflect padding, power 1)
 *   gsv_ref_get_ge          SynthesizerTrn.get_ge (SoVITS/models.py:371-378): ref_enc = MelStyleEncoder
 *                           (module/modules.py:367-444) on refer[:, :704], + sv_emb(sv) and PReLU for v2Pro / v2ProPlus
 *   gsv_ref_extract_latent  SynthesizerTrn.extract_latent (models.py:431-434): ssl_proj (k 2, stride 2) and the
 *                           nearest-codebook search of EuclideanCodebook.quantize (module/core_vq.py:124-128)
 * Tensors ("ref_enc.*", "sv_emb.*", "prelu.weight", "ssl_proj.*", "quantizer.vq.layers.0._codebook.embed") are
 * given under their checkpoint names, device fp32, before finalize.  `ssl` comes from CN-HuBERT (gsv_hubert_* below),
 * `sv_emb` from ERes2NetV2 (gsv_sv_* below); audio decoding is outside this library. */
typedef struct gsv_ref gsv_ref;
typedef struct gsv_ref_config {
    int n_fft;      /* hps.data.filter_length == win_length (2048) */
    int hop;        /* hps.data.hop_length (640) */
    int spec_bins;  /* spectrogram bins ref_enc reads (704, models.py:305,373) */
    int hidden;     /* MelStyleEncoder style_hidden (128) */
    int n_head;     /* 2 */
    int kernel;     /* Conv1dGLU kernel (5) */
    int gin;        /* gin_channels: 512 (v2) / 1024 (v2Pro, v2ProPlus) */
    int sv_dim;     /* 20480 for v2Pro / v2ProPlus, 0 for v2 (no sv_emb / prelu) */
    int ssl_dim;    /* 768 */
    int bins;       /* codebook size (1024) */
} gsv_ref_config;
int gsv_ref_create(const gsv_ref_config* cfg, gsv_ref** out);
int gsv_ref_destroy(gsv_ref* h);
int gsv_ref_load_tensor(gsv_ref* h, const char* name, const float* data, int64_t numel, void* stream);
int gsv_ref_finalize(gsv_ref* h, void* stream);
/* bytes that cover a spectrogram of n_samples, a get_ge of n_frames and an extract_latent of n_ssl (0 = not used) */
size_t gsv_ref_workspace(gsv_ref* h, int n_samples, int n_frames, int n_ssl);
/* audio fp32 [n_samples] (mono, at the model rate) -> spec fp32 [n_fft/2+1][1 + n_samples/hop], channels-first */
int gsv_ref_spectrogram(gsv_ref* h, const float* audio, int n_samples, float* spec, void* workspace, size_t workspace_bytes,
                        void* stream);
/* spec fp32 [>= spec_bins][n_frames] channels-first (row stride n_frames), sv_emb fp32 [sv_dim] or NULL -> ge fp32 [gin] */
int gsv_ref_get_ge(gsv_ref* h, const float* spec, int n_frames, const float* sv_emb, float* ge, void* workspace,
                   size_t workspace_bytes, void* stream);
/* ssl fp32 [ssl_dim][n_ssl] channels-first (CN-HuBERT last_hidden_state transposed, TTS.py:1567) -> codes int64
 * [n_ssl/2]; margin fp32 [n_ssl/2] or NULL = distance gap between the best and the second-best code */
int gsv_ref_extract_latent(gsv_ref* h, const float* ssl, int n_ssl, int64_t* codes, float* margin, void* workspace,
                           size_t workspace_bytes, void* stream);

/* CN-HuBERT, once per new prompt: HubertModel(wav16k)["last_hidden_state"] as TTS._get_prompt calls it
 * (gsv_tts/TTS.py:1556-1570; GPT_SoVITS/Featurizer/cnhubert.py wraps transformers.HubertModel), fp32 in every mode.
 * The configuration HubertConfig() describes (feat_extract_norm "group", do_stable_layer_norm False, no conv bias, exact
 * GELU) is the only one: feature encoder (conv 0 + GroupNorm over all frames, strided convs), LayerNorm + projection,
 * grouped positional conv with weight norm (dim 2), encoder.layer_norm, post-LN transformer layers (no mask, batch 1).
 * Tensors under their Hugging Face state-dict names ("feature_extractor.*", "feature_projection.*", "encoder.*"), device
 * fp32, before finalize; the positional conv's weight norm is accepted as weight_g / weight_v or as
 * parametrizations.weight.original0 / original1 and folded at finalize.  Resampling to 16 kHz is the caller's. */
typedef struct gsv_hubert gsv_hubert;
#define GSV_HUBERT_MAX_CONV 8
typedef struct gsv_hubert_config {
    int hidden;                           /* hidden_size (768); head dim hidden / n_head must be 64 */
    int n_layer;                          /* num_hidden_layers (12) */
    int n_head;                           /* num_attention_heads (12) */
    int ffn;                              /* intermediate_size (3072) */
    int n_conv;                           /* len(conv_dim) (7) */
    int conv_dim[GSV_HUBERT_MAX_CONV];    /* 512 each; multiples of 64, <= 1024 */
    int conv_kernel[GSV_HUBERT_MAX_CONV]; /* 10, 3, 3, 3, 3, 2, 2 */
    int conv_stride[GSV_HUBERT_MAX_CONV]; /* 5, 2, 2, 2, 2, 2, 2 */
    int pos_k;                            /* num_conv_pos_embeddings (128, even) */
    int pos_groups;                       /* num_conv_pos_embedding_groups (16) */
    float eps;                            /* layer_norm_eps (1e-5); GroupNorm keeps torch's 1e-5 */
} gsv_hubert_config;
/* refuses (GSV_ERR_ARG, gsv_last_error says why) any shape the kernels do not support */
int gsv_hubert_create(const gsv_hubert_config* cfg, gsv_hubert** out);
int gsv_hubert_destroy(gsv_hubert* h);
int gsv_hubert_load_tensor(gsv_hubert* h, const char* name, const float* data, int64_t numel, void* stream);
int gsv_hubert_finalize(gsv_hubert* h, void* stream);
/* output frames Th for n_samples: T0 = (n - k0) / s0 + 1, Ti = (T(i-1) - ki) / si + 1; 0 when the input is too short
 * (fewer than 400 samples for the default shapes) */
int gsv_hubert_frames(gsv_hubert* h, int n_samples);
/* device bytes of the caller-owned workspace of one forward over n_samples; 0 when n_samples is too short */
size_t gsv_hubert_workspace(gsv_hubert* h, int n_samples);
/* audio fp32 [n_samples] (mono, 16 kHz, as the model reads it: no normalisation) -> ssl fp32 [hidden][Th] channels-first
 * (last_hidden_state transposed, what gsv_ref_extract_latent takes).  Nothing is allocated. */
int gsv_hubert_forward(gsv_hubert* h, const float* audio, int n_samples, float* ssl, void* workspace, size_t workspace_bytes,
                       void* stream);
/* Batches of CN-HuBERT / ERes2NetV2 clips: up to GSV_AUX_MAX_CLIPS clips in one call, each clip's output bit-identical to
 * the single-clip call on that clip whatever else is in the batch and in any order.  n_samples / n_frames are HOST arrays
 * of n_clips; nothing is allocated or copied from the host inside the calls.  GSV_ERR_ARG (gsv_last_error names the clip)
 * for n_clips outside 1..GSV_AUX_MAX_CLIPS, a clip too short, a bad rate, a workspace too small or not 16-byte aligned. */
#define GSV_AUX_MAX_CLIPS 64
/* device bytes of the workspace of gsv_hubert_forward_batch over these clips; 0 when a clip is too short */
size_t gsv_hubert_batch_workspace(gsv_hubert* h, const int* n_samples, int n_clips);
/* audio: the clips' 16 kHz samples back to back; ssl: clip i's [hidden][Th_i] block at offset hidden * sum_{j<i} Th_j */
int gsv_hubert_forward_batch(gsv_hubert* h, const float* audio, const int* n_samples, int n_clips, float* ssl,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ERes2NetV2, once per new speaker: the speaker-verification embedding sv_emb that get_ge adds for v2Pro / v2ProPlus, as
 * TTS.cache_spk_audio computes it (gsv_tts/TTS.py:1346-1389, 1591-1610; GPT_SoVITS/SV/sv.py): the model-rate waveform
 * resampled to 16 kHz (torchaudio Resample defaults), an 80-bin Kaldi fbank (dither 0), then
 * ERes2NetV2(baseWidth=24, scale=4, expansion=4).forward3, fp32 in every mode.  Tensors under the checkpoint's
 * state-dict names ("conv1.*", "bn1.*", "layer1..4.*", "layer3_ds.*", "fuse34.*"), device fp32, before finalize; BN
 * (eval, eps 1e-5) is folded at finalize.  seg_1.*, pool.* and num_batches_tracked are not read by forward3: leave them
 * out.  Bit-reproducible (no atomics). */
typedef struct gsv_sv gsv_sv;
typedef struct gsv_sv_config {
    int m_channels;   /* stem channels (64); stage s has planes m_channels << s and 4 * planes output channels */
    int blocks[4];    /* blocks per stage ([3, 4, 6, 3]) */
    int width[4];     /* Res2Net split width per stage, floor(planes * baseWidth / 64) (24, 48, 96, 192); >= 4 */
    int scale;        /* splits per block: 4 only */
    int expansion;    /* 4 only */
    int feat_dim;     /* fbank bins: 80 only */
} gsv_sv_config;
/* refuses (GSV_ERR_ARG) any other scale, expansion or feat_dim */
int gsv_sv_create(const gsv_sv_config* cfg, gsv_sv** out);
int gsv_sv_destroy(gsv_sv* h);
int gsv_sv_load_tensor(gsv_sv* h, const char* name, const float* data, int64_t numel, void* stream);
int gsv_sv_finalize(gsv_sv* h, void* stream);
/* ceil(new * n / orig) with the rates reduced by their gcd (n when the rates are equal); 0 on bad arguments */
int gsv_sv_resample_length(int n_samples, int orig_sr, int new_sr);
/* device bytes gsv_sv_resample needs for this rate pair (its fp32 kernel table) */
size_t gsv_sv_resample_workspace(int orig_sr, int new_sr);
/* torchaudio.transforms.Resample(orig_sr, new_sr) with default arguments: x fp32 [n] -> y fp32
 * [gsv_sv_resample_length(n, orig_sr, new_sr)].  Needs no model handle. */
int gsv_sv_resample(const float* x, int n_samples, int orig_sr, int new_sr, float* y, void* workspace, size_t workspace_bytes,
                    void* stream);
/* Reference-audio files: the samples of a WAV data chunk, copied to the device as they are in the file (interleaved
 * little-endian frames), -> fp32 mono, what TTS._load_audio gets from av.AudioResampler(format='flt', layout='mono')
 * (gsv_tts/TTS.py:1811-1823).  u8 (x - 128) / 2^7, s16 x / 2^15, packed s24 x / 2^23, s32 x / 2^31, f32 as is, f64 cast
 * to float; 1 or 2 channels, stereo mixed as (L + R) * sqrt(1/2).  Needs no model handle, allocates
 * nothing, reads no alignment into pcm.  The host parses the RIFF container (gsv_tts_lite_amd/wavio.py). */
#define GSV_PCM_U8 0
#define GSV_PCM_S16 1
#define GSV_PCM_S24 2
#define GSV_PCM_S32 3
#define GSV_PCM_F32 4
#define GSV_PCM_F64 5
/* pcm: pcm_bytes device bytes holding n_frames frames of `channels` samples of `format` from byte 0 -> out fp32
 * [n_frames].  GSV_ERR_ARG for an unknown format, channels outside 1..2, n_frames < 1 or frames past pcm_bytes. */
int gsv_wav_to_mono(const void* pcm, size_t pcm_bytes, int n_frames, int format, int channels, float* out, void* stream);
/* one clip of gsv_wav_to_mono_batch: its frames start at byte_offset of the packed pcm */
typedef struct gsv_wav_clip {
    int64_t byte_offset;
    int32_t n_frames;
    int16_t format;     /* GSV_PCM_* */
    int16_t channels;   /* 1 or 2 */
} gsv_wav_clip;
/* up to GSV_AUX_MAX_CLIPS clips (a HOST array) in one launch: out holds clip i's [n_frames_i] at offset
 * sum_{j<i} n_frames_j, bit-identical to gsv_wav_to_mono on that clip.  GSV_ERR_ARG names the first bad clip. */
int gsv_wav_to_mono_batch(const void* pcm, size_t pcm_bytes, const gsv_wav_clip* clips, int n_clips, float* out, void* stream);
/* Reference-audio files, FLAC: the frames of up to GSV_AUX_MAX_CLIPS files, packed into one device byte buffer, decoded
 * on the device (csrc/flacdec.h: one lane per frame) into interleaved s32 staging, left-justified, which the WAV path's
 * own conversion (GSV_PCM_S32) then turns into fp32 mono: a FLAC clip is bit-identical to the WAV file holding the same
 * integers.  1 or 2 channels, 8..24 bits per sample.  The host parses the container and indexes the frames
 * (gsv_tts_lite_amd/flacio.py); the tables below are HOST arrays, read before the call returns. */
typedef struct gsv_flac_clip {
    int32_t channels;          /* 1 or 2 */
    int32_t bits_per_sample;   /* 8..24, from STREAMINFO */
    int32_t n_samples;         /* per channel */
    int32_t reserved;
    int64_t out_offset;        /* of the clip's fp32 mono samples in `out`, in samples */
} gsv_flac_clip;
typedef struct gsv_flac_frame {
    int32_t clip;              /* index into the clip table */
    int32_t block_size;        /* samples per channel in this frame, 1..65535 */
    int64_t byte_offset;       /* of the frame's sync code in the packed bytes */
    int32_t byte_len;          /* through its CRC-16; with GSV_FLAC_OPEN_END an upper bound */
    int32_t first_sample;      /* within the clip */
    int32_t flags;             /* GSV_FLAC_OPEN_END or 0 */
    int32_t reserved;
} gsv_flac_frame;
/* a file's last frame: no header follows it, so the host cannot know where it ends (bytes may trail it).  The decoder
 * then reads the CRC-16 from where the frame's structure ends, anywhere inside byte_len. */
#define GSV_FLAC_OPEN_END 1
/* status codes a frame can end with (status[i] of frame i; a failed frame's samples are zero) */
#define GSV_FLAC_OK 0
#define GSV_FLAC_OVERRUN 1      /* the frame's structure needs more bits than byte_len holds */
#define GSV_FLAC_SYNC 2         /* no sync code, or a reserved header bit */
#define GSV_FLAC_RESERVED 3     /* a reserved code */
#define GSV_FLAC_CRC8 4         /* header CRC-8 mismatch */
#define GSV_FLAC_MISMATCH 5     /* header disagrees with the tables (block size, channels, bits per sample) */
#define GSV_FLAC_ORDER 6        /* predictor order larger than the block */
#define GSV_FLAC_PARTITION 7    /* residual partitions do not divide the block */
#define GSV_FLAC_RESIDUAL 8     /* residual outside 32 bits */
#define GSV_FLAC_RANGE 9        /* sample outside the stream's bits per sample */
#define GSV_FLAC_LENGTH 10      /* the structure ends before byte_len - 2 */
#define GSV_FLAC_CRC16 11       /* frame CRC-16 mismatch */
#define GSV_FLAC_WASTED 12      /* wasted bits leave no bit of the sample */
/* device bytes of the workspace of gsv_flac_decode (the device frame table + the s32 staging); 0 on bad arguments */
size_t gsv_flac_decode_workspace(const gsv_flac_clip* clips, int n_clips, int n_frames);
/* bytes: n_bytes DEVICE bytes; out: fp32, clip c at out_offset_c .. + n_samples_c; status_dev: int32 [n_frames] on the
 * device.  Checked before anything is launched, each GSV_ERR_ARG with gsv_last_error naming the first bad entry: 1..
 * GSV_AUX_MAX_CLIPS clips, channels 1 or 2, bits 8..24, every frame inside n_bytes, the frames of each clip (in table
 * order) tiling [0, n_samples) exactly, the workspace large enough and 16-byte aligned.  One table upload and two
 * launches (frames, mono conversion) on `stream`; nothing is allocated. */
int gsv_flac_decode(const void* bytes_dev, size_t n_bytes, const gsv_flac_clip* clips, int n_clips,
                    const gsv_flac_frame* frames, int n_frames, float* out, int32_t* status_dev, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The same frame routine run by the CPU over HOST memory, for tests and tools (not an inference path): the integers as
 * they were encoded (right-justified), interleaved, clip c at sum_{j<c} n_samples_j * channels_j of pcm_interleaved;
 * status: int32 [n_frames].  The same argument checks; out_offset is not used.  Needs no GPU. */
int gsv_flac_decode_host(const void* bytes, size_t n_bytes, const gsv_flac_clip* clips, int n_clips,
                         const gsv_flac_frame* frames, int n_frames, int32_t* pcm_interleaved, int32_t* status);
/* Writing FLAC: mono fp32 clips -> frames of native FLAC with fixed blocking at 16 or 24 bits per sample, encoded on the
 * device (csrc/flacenc.h: one wave per frame).  The encoding has one right answer: the quantiser
 * q = clamp(rint(x * 2^(bits-1))) with NaN -> 0; per frame CONSTANT when all samples are equal, else the FIXED order 0..4
 * and Rice partition order 0..6 (each partition's best parameter, no escapes) with the fewest bits -- ties to the lower
 * order, then the lower partition order -- or VERBATIM when that is strictly smaller.  The host builds the container and
 * every frame's header, CRC-8 included (gsv_tts_lite_amd/flacio.py); the device copies the header in front of the
 * subframe and closes the frame with its CRC-16.  The tables below are HOST arrays, read before the call returns. */
typedef struct gsv_flac_enc_clip {
    int64_t in_offset;         /* of the clip's first sample in `samples`, in samples */
    int32_t n_samples;
    int32_t bits_per_sample;   /* 16 or 24 */
} gsv_flac_enc_clip;
typedef struct gsv_flac_enc_frame {
    int32_t clip;              /* index into the clip table */
    int32_t block_size;        /* samples in this frame, 1..4608 */
    int32_t first_sample;      /* within the clip */
    int32_t header_len;        /* 6..16 bytes of `header`, through the CRC-8 */
    uint8_t header[16];
} gsv_flac_enc_frame;
#define GSV_FLAC_ENC_CONSTANT 0
#define GSV_FLAC_ENC_VERBATIM 1
#define GSV_FLAC_ENC_FIXED 2
/* what a frame was coded with: kind GSV_FLAC_ENC_*; for FIXED the predictor order, the partition order, the residual
 * method (0 at 16 bits, 1 at 24) and k[j], partition j's Rice parameter for j < 2^porder; every other field 0 */
typedef struct gsv_flac_enc_choice {
    uint8_t kind, order, porder, method;
    uint8_t k[64];
} gsv_flac_enc_choice;
/* the most bytes the frames of a table can take (every frame VERBATIM): what out_bytes must hold; 0 on bad arguments */
size_t gsv_flac_encode_bound(const gsv_flac_enc_clip* clips, int n_clips, const gsv_flac_enc_frame* frames, int n_frames);
/* device bytes of the workspace of gsv_flac_encode (the device frame table, one worst-case slot per frame, the
 * lengths); 0 on bad arguments */
size_t gsv_flac_encode_workspace(const gsv_flac_enc_clip* clips, int n_clips, const gsv_flac_enc_frame* frames, int n_frames);
/* samples_dev: n_samples fp32 on the DEVICE; out_dev: the frames packed back to back, in table order; frame_offsets_dev:
 * int64 [n_frames + 1] on the device, frame f at out_dev[frame_offsets[f], frame_offsets[f + 1]); choices_dev: [n_frames]
 * on the device, or NULL.  Checked before anything is launched, each GSV_ERR_ARG with gsv_last_error naming the first bad
 * entry: 1..GSV_AUX_MAX_CLIPS clips, each inside n_samples, bits 16 or 24, block sizes 1..4608, header_len 6..16, the
 * frames of each clip (in table order) tiling [0, n_samples) exactly, out_bytes at least gsv_flac_encode_bound, the
 * workspace large enough and 16-byte aligned.  One table upload and three launches (frames, scan, copy) on `stream`;
 * no device memory is allocated (the device table is staged in a host vector).  The encoder has no data-dependent failure. */
int gsv_flac_encode(const float* samples_dev, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                    const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out_dev, size_t out_bytes,
                    int64_t* frame_offsets_dev, gsv_flac_enc_choice* choices_dev, void* workspace, size_t workspace_bytes,
                    void* stream);
/* The same over HOST memory, frame after frame on the CPU from the same scalar pieces: the CPU path of flacio.encode_flacs
 * and the device's oracle (device bytes equal host bytes).  The same argument checks; needs no GPU. */
int gsv_flac_encode_host(const float* samples, size_t n_samples, const gsv_flac_enc_clip* clips, int n_clips,
                         const gsv_flac_enc_frame* frames, int n_frames, uint8_t* out, size_t out_bytes,
                         int64_t* frame_offsets, gsv_flac_enc_choice* choices);
/* fbank frames of a waveform of n_samples at sample_rate once it is at 16 kHz: 1 + (n16 - 400) / 160, 0 if n16 < 400 */
int gsv_sv_frames(gsv_sv* h, int n_samples, int sample_rate);
/* device bytes of the caller-owned workspace of gsv_sv_embed over n_samples at sample_rate; it also covers
 * gsv_sv_resample of that input, and gsv_sv_fbank / gsv_sv_forward of what it resamples to.  0 when too short. */
size_t gsv_sv_workspace(gsv_sv* h, int n_samples, int sample_rate);
/* wav fp32 [n_samples] at 16 kHz -> feat fp32 [frames][80], Kaldi.fbank(num_mel_bins=80, sample_frequency=16000, dither=0) */
int gsv_sv_fbank(gsv_sv* h, const float* wav16k, int n_samples, float* feat, void* workspace, size_t workspace_bytes,
                 void* stream);
/* feat fp32 [n_frames][80] -> sv_emb fp32 [4 * 8 * m_channels * 10] = forward3(feat[None]), index c * 10 + f */
int gsv_sv_forward(gsv_sv* h, const float* feat, int n_frames, float* sv_emb, void* workspace, size_t workspace_bytes,
                   void* stream);
/* wav fp32 [n_samples] at sample_rate (mono, peak-normalised by the caller) -> resample to 16 kHz -> fbank -> sv_emb */
int gsv_sv_embed(gsv_sv* h, const float* wav, int n_samples, int sample_rate, float* sv_emb, void* workspace,
                 size_t workspace_bytes, void* stream);
/* Batches (GSV_AUX_MAX_CLIPS, see gsv_hubert_forward_batch): device bytes of the workspace of gsv_sv_embed_batch over
 * these clips at sample_rate; it also covers gsv_sv_forward_batch of clips whose equivalent 16 kHz lengths
 * 400 + 160 * (n_frames - 1) are given at 16000.  0 on bad arguments. */
size_t gsv_sv_batch_workspace(gsv_sv* h, const int* n_samples, int n_clips, int sample_rate);
/* feat: the clips' [n_frames_i][80] fbank rows back to back -> sv_emb [n_clips][emb_dim] (forward3 of each clip) */
int gsv_sv_forward_batch(gsv_sv* h, const float* feat, const int* n_frames, int n_clips, float* sv_emb,
                         void* workspace, size_t workspace_bytes, void* stream);
/* wav: the clips back to back at sample_rate (peak-normalised by the caller) -> sv_emb [n_clips][emb_dim] */
int gsv_sv_embed_batch(gsv_sv* h, const float* wav, const int* n_samples, int n_clips, int sample_rate, float* sv_emb,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Chinese RoBERTa, once per request: hidden_states[-3] of BertForMaskedLM (chinese-roberta-wwm-ext-large) and the
 * phone features CNRoberta._forward_pytorch builds from them (gsv_tts/GPT_SoVITS/Featurizer/cnroberta.py), fp32 in every
 * mode.  Absolute positions, exact GELU, post-LN layers; only encoder.layer.0 .. n_layer-3 run (hidden_states[-3] is
 * their output; the embeddings' LayerNorm when n_layer == 2).  Tensors under their Hugging Face names without the
 * "bert." prefix ("embeddings.*", "encoder.layer.{l}.*"), device fp32, before finalize; the last two layers, the pooler
 * and cls.* are refused.  Texts run packed: ids int32 [total_rows] holds every text's [CLS] .. [SEP] ids back to back,
 * seq_starts int32 [n_seq + 1] (device) delimits them, positions restart at every text and token type is 0.  A text's
 * rows are bit-identical whatever else is in the batch, and two calls are bit-identical (no atomics). */
typedef struct gsv_roberta gsv_roberta;
typedef struct gsv_roberta_config {
    int hidden;       /* hidden_size (1024); a multiple of 64, <= 1024, head dim hidden / n_head must be 64 */
    int n_layer;      /* num_hidden_layers (24), >= 2; n_layer - 2 of them run */
    int n_head;       /* num_attention_heads (16) */
    int ffn;          /* intermediate_size (4096), a multiple of 64 */
    int vocab;        /* vocab_size (21128) */
    int max_pos;      /* max_position_embeddings (512): the longest text, [CLS] and [SEP] included */
    int type_vocab;   /* type_vocab_size (2); row 0 is added */
    float eps;        /* layer_norm_eps (1e-12) */
} gsv_roberta_config;
/* refuses (GSV_ERR_ARG, gsv_last_error says why) any shape the kernels do not support */
int gsv_roberta_create(const gsv_roberta_config* cfg, gsv_roberta** out);
int gsv_roberta_destroy(gsv_roberta* h);
int gsv_roberta_load_tensor(gsv_roberta* h, const char* name, const float* data, int64_t numel, void* stream);
int gsv_roberta_finalize(gsv_roberta* h, void* stream);
/* device bytes of the caller-owned workspace of one call over total_rows packed rows of n_seq texts, the longest
 * max_len rows; 0 on bad arguments */
size_t gsv_roberta_workspace(gsv_roberta* h, int total_rows, int n_seq, int max_len);
/* ids, seq_starts as above (2 <= every length <= max_len <= max_pos) -> hidden_out fp32 [total_rows][hidden] =
 * hidden_states[-3] at every packed row.  Nothing is allocated. */
int gsv_roberta_forward(gsv_roberta* h, const int* ids, const int* seq_starts, int n_seq, int total_rows, int max_len,
                        float* hidden_out, void* workspace, size_t workspace_bytes, void* stream);
/* the same forward, then out fp32 [n_phones][hidden] = hidden row phone_index[p] (int32, device): the host builds the
 * index from word2ph["ph"], skipping every text's [CLS] and [SEP] rows and repeating the others. */
int gsv_roberta_features(gsv_roberta* h, const int* ids, const int* seq_starts, int n_seq, int total_rows, int max_len,
                         const int* phone_index, int n_phones, float* out, void* workspace, size_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSV_TTS_HIP_H */
