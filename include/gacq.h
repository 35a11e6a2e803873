/* gacq.h -- C ABI of the MI355X-native GNSS acquisition engine (libgacq.so).
 *
 * This is the drop-in boundary for ONE hot path of pmonta/GNSS-DSP-tools: the FFT-based parallel
 * code-phase search that every acquire-*.py defines inline as
 *     search(x, prn, doppler_search, ms) -> (metric, code, doppler)      acquire-gps-l1.py:18-40
 * The reference has no FFI of its own (pure Python); the entry points below are what a ctypes
 * binding for that function needs, and gnss-dsp-tools_amd/acquire.py is that binding
 * (INTEGRATION.md shows the stub a maintainer would drop into acquire-gps-l1.py).
 *
 * Conventions: plain pointers and sizes only; every function returns GACQ_OK (0) or a negative
 * GACQ_ERR_* code and never throws across the ABI; gacq_last_error() gives the message.
 * Host buffers are caller-owned; device buffers passed to *_dev entry points are caller-owned
 * device pointers (e.g. torch tensors' data_ptr()); everything else on the device is library-owned.
 * A gacq_ctx is bound to one HIP device and is single-threaded; a gacq_group drives several devices from one thread.
 */
#ifndef GACQ_H
#define GACQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GACQ_OK 0
#define GACQ_ERR_BAD_ARG (-1)
#define GACQ_ERR_UNKNOWN_CODE (-2)
#define GACQ_ERR_BAD_PRN (-3)
#define GACQ_ERR_HIP (-4)
#define GACQ_ERR_ROCFFT (-5)
#define GACQ_ERR_SHORT_INPUT (-6)
#define GACQ_ERR_NO_DEVICE (-7)
#define GACQ_ERR_INTERNAL (-8)
#define GACQ_ERR_UNSUPPORTED (-9)
/* Positive: the call succeeded and its results are valid, with a caveat.  gacq_search / gacq_search64 (the calls that wait for their
 * results) return this when the call's tie-safe re-evaluation list was too small (GACQ_OPT_TIE_CAP): every ambiguous pair of the call
 * kept its fp32 location.  The asynchronous device-buffer calls cannot report it (an overflow of theirs is reported by the next
 * gacq_search / gacq_search64 on the same context, or poll gacq_get_tie_stats()[2] after synchronising); gacq_search_batch and the
 * gacq_group_* calls do not return it either. */
#define GACQ_WARN_TIE_LIST_FULL 1

/* ---------------------------------------------------------------------------------------------
 * PRN chip generators (host only, no GPU needed).  `code` is the reference module name:
 * "gps.ca" == gnsstools/gps/ca.py, "galileo.e1b", "beidou.b1i", "glonass.ca", ...
 * Replaces: <module>.<sig>_code(prn) and <module>.code(prn,0,0,L/n,n)  (gnsstools/gps/ca.py:101-112)
 *           nco.boc11(0,0,L/n,n)                                         (gnsstools/nco.py:12-19)
 * ------------------------------------------------------------------------------------------- */
int gacq_code_count(void);
const char* gacq_code_name(int index);
int gacq_code_length(const char* code);                 /* chips, or GACQ_ERR_UNKNOWN_CODE */
double gacq_code_chip_rate(const char* code);
int gacq_code_prns(const char* code, int* out, int cap);/* returns number of valid PRNs */
int gacq_code_chips(const char* code, int prn, uint8_t* out, int cap);   /* {0,1} per chip */
int gacq_code_replica(const char* code, int prn, int n, int boc, float* out); /* +-1 samples */

/* ---------------------------------------------------------------------------------------------
 * Acquisition engine.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_ctx gacq_ctx;
typedef struct gacq_sig gacq_sig;

/* The six knobs that distinguish the 28 FFT search() variants. */
typedef struct gacq_sigdesc {
  int code_length;   /* chips in one code period                      (ca.code_length)            */
  int n;             /* samples per coherent block at the internal fs (acquire-gps-l1.py:20)      */
  int pad;           /* 1: replica zero-extended to N=2n, windows x[b*n:(b+2)*n]                  */
                     /*    (acquire-beidou-b1i.py:24,30); 0: N=n (acquire-gps-l1.py:24,30)        */
  int boc;           /* 1: replica multiplied by nco.boc11 (acquire-galileo-e1b.py:25-26)         */
  int metric_mode;   /* 1: max/mean (acquire-gps-l1.py:35); 0: raw max (acquire-beidou-b1i.py:36) */
  int fold_code;     /* 1: code phase reported modulo code_length (acquire-beidou-b1i.py:39)      */
  double fs;         /* internal sampling rate in Hz                  (acquire-gps-l1.py:19)      */
} gacq_sigdesc;

/* Final per-item answer == the reference's return tuple (acquire-gps-l1.py:40), plus raw indices. */
typedef struct gacq_result {
  double metric;      /* m_metric                                                    */
  double code_chips;  /* m_code   = code_length*(float(idx)/n) [% code_length]       */
  double doppler_hz;  /* m_doppler                                                   */
  int idx;            /* argmax lag of the winning Doppler bin (-1 if no bin won)    */
  int d_index;        /* index of the winning bin in the Doppler grid (-1 if none)   */
} gacq_result;

/* Device-side record: best over a (local) Doppler slice for one (epoch, item). 16 bytes.
 * This is what crosses GPUs (one gather of these). */
typedef struct gacq_peak {
  double metric;      /* 0.0 when nothing beat the initial m_metric = 0 (acquire-gps-l1.py:25) */
  int idx;
  int d_index;
} gacq_peak;

int gacq_device_count(void);
int gacq_create(int device_id, gacq_ctx** out);
void gacq_destroy(gacq_ctx* ctx);
const char* gacq_last_error(gacq_ctx* ctx);             /* ctx may be NULL: last global error */

/* Use the caller's HIP stream (hipStream_t passed as void*; NULL = the ctx-owned stream). */
int gacq_set_stream(gacq_ctx* ctx, void* hip_stream);
/* Launch on the legacy default ("null") stream -- what torch.cuda.current_stream() is unless the caller
 * entered a stream context; needed so that work is ordered with collectives issued on that stream. */
int gacq_use_null_stream(gacq_ctx* ctx);
/* Engine selection: 0 = auto, 1 = rocFFT pipeline (any N), 2 = LDS-resident FFT kernels (N = 4096, 16384),
 * 3 = split engine, outer radix 31/16/4: prime-factor form for N = 61380 / 30690, rocFFT inner transforms otherwise (65536, 16384, ...),
 * 4 = split engine with the inner transforms on the LDS FFT kernels (N = 65536, 16384),
 * 5 = complex128 engine (any N): every value in fp64 on the device, as the reference computes (numpy complex128); agrees with it
 *     to ~1e-12 and is what a near-tie disagreement of an fp32 engine is bisected against.  N = 4096 with one block and one carrier
 *     runs as ONE fused kernel (fp64 transform resident in LDS), with several blocks or carriers as a forward + a correlate kernel on the
 *     same transform; N = 16384 and 65536 (B1I / B2I, GLONASS, E1B / E1C) as the split
 *     form 4 x / 16 x 4096 on the same transform -- forward spectra shared by the items, one Z' round trip of 32 N bytes per row and
 *     block, no rocFFT plan; N = 61380 / 30690 (the 10.23 Mcps scripts, E6, Xona X5) as 31 x M with hand-written fp64 DFT-31 stages
 *     around rocFFT's native length-M double transforms, which keeps the prime 31 out of rocFFT's Bluestein path (all three:
 *     GACQ_OPT_FUSED_C128); every other shape as the five-stage pipeline on rocFFT's double-precision transforms.  Never chosen by auto. */
int gacq_set_engine(gacq_ctx* ctx, int engine);
/* Upper bound in bytes for EACH of the two library-owned work buffers of a context -- the forward spectra and the correlation workspace;
 * both are allocated as searches need them, with 1/8 of headroom, and kept, so a context can hold about 2.25 x this (default 32 GiB
 * of the part's 288 GB).  A search whose forward spectra for one epoch exceed it is cut into Doppler slices that fit; the slices are
 * merged in grid order with strict '>' (acquire-gps-l1.py:36-39), so the result is the one of a single scan.  Until this is called the
 * library also keeps each buffer within the context's share of the device's FREE memory (80 % of it, split over the contexts alive on
 * the device and their two buffers each), so that several contexts, ranks or a torch allocator sharing a device cannot over-commit it;
 * a limit set here is taken as given.  Either way a search whose workspace cannot be allocated is re-run in passes of half the size
 * (down to 64 MiB) before an error is returned.  One pass of the split engines' correlation workspace is at most 4 GiB or eight
 * items' worth, whichever is more: the limit is the ceiling of a pass, not its size. */
int gacq_set_workspace_limit(gacq_ctx* ctx, size_t bytes);
/* Tuning switches of the launch path.  They are ctx state set through this call; nothing in the library reads the
 * environment.  Defaults in brackets. */
#define GACQ_OPT_FUSED_INNER 0  /* [1] engine 3, N = 61380 / 30690: 1 = prime-factor form (no twiddles at any level, conj-multiply fused into the */
                                /*     in-place inner inverse transforms; gacq_pfa.hip); 0 = Cooley-Tukey form with rocFFT inner transforms    */
                                /*     (other arithmetic: the cross-check)                                                                     */
#define GACQ_OPT_FUSED_16K 1    /* [1] N = 16384 with one carrier per item: forward + correlate in one kernel           */
#define GACQ_OPT_LDS_VARIANT 2  /* [-1] N = 16384: 16 = the radix-16 form of the one-workgroup transform (1024 threads x 16 points, three     */
                                /*     exchanges; gacq_lds16k_r16.hip) instead of the radix-32 form (512 x 32, two exchanges; gacq_lds16k.hip). */
                                /*     Same results to fp32 rounding; the radix-32 form issues 13 % fewer VALU instructions at half the waves  */
                                /*     and measures 0-5 % faster on B1I, within 2 % on GLONASS (the in-run A/B of bench.py); other values: radix-32 form                */
#define GACQ_OPT_LDS_PCH 3      /* [0 = auto] items per workgroup of the LDS correlate kernels                          */
#define GACQ_OPT_SPLIT_PCH 4    /* [0 = auto] (epoch, item) rows per workgroup of the split engines' inner kernels      */
#define GACQ_OPT_SPLIT_TEAMS 5  /* retired (round 5): belonged to the Stockham inner kernel the prime-factor engine replaced; accepted, ignored */
#define GACQ_OPT_FUSED_4K 6     /* [1] N = 4096, B = 1, one carrier, >= 1024 (epoch, Doppler) units: forward + correlate in  */
                                /*     one kernel (no forward-spectra buffer); 2 = also for small batches                    */
#define GACQ_OPT_SPLIT_DT 7      /* [0 = auto] Doppler bins per workgroup of the prime-factor engine's inner kernel (1, 2 or 3): every   */
                                /*     code-spectrum row fetched serves that many correlation rows                                         */
#define GACQ_OPT_FE_GENERIC 8    /* [0] front-end: 1 = run the any-length mix + FIR kernels even for the reference's 161-tap filter     */
                                /*     (the specialised kernels produce the same bits; this is the A/B and test switch)              */
#define GACQ_OPT_LDS_UGROUP 9    /* [0 = auto, <= 64] N = 16384 correlate kernel: (epoch, Doppler) units a workgroup walks with one item's  */
                                /*     code spectrum held in registers (round 4: item-major order; the spectrum is fetched once per group)  */
#define GACQ_OPT_SEARCH1 10       /* retired (round 6): the single-launch search of round 3 (Doppler scan inside the correlate kernel) measured     */
                                /*     slower than three short launches and had no tie-safe re-evaluation; removed.  Accepted, ignored             */
#define GACQ_OPT_BAR_UPLOAD 11    /* [1] gacq_search: inputs up to 256 KiB are written by the host straight into fine-grained device       */
                                /*     memory through the PCIe BAR (large-BAR devices) instead of pinned staging + DMA                  */
#define GACQ_OPT_WATCH_RESULTS 12 /* [1] gacq_search (BAR upload path only): wait for completion by watching the pinned result records for  */
                                /*     the last kernel's stores (bounded spin, then hipStreamSynchronize) instead of a runtime sync          */
#define GACQ_OPT_TIE_SAFE 13      /* [1] tie-safe peak locations: every (epoch, item) whose winning lag or Doppler bin has a runner-up    */
                                /*     within GACQ_OPT_TIE_EPS_PPB of it is re-evaluated in complex128 on the device (the reference's     */
                                /*     arithmetic type, acquire-gps-l1.py:30-39) before its record is written, so the reported location is */
                                /*     the complex128 one and not whichever side of a near-tie the fp32 rounding fell on                   */
#define GACQ_OPT_TIE_EPS_PPB 14   /* [8000] relative gap, in parts per billion, below which two magnitudes / metrics count as tied         */
                                /*     (8e-6 ~ 6 x the worst fp32-vs-complex128 metric error observed); 1000000000 re-evaluates every row  */
#define GACQ_OPT_TIE_CAP 15       /* [0 = auto: 64 + (epochs x items) / 16] rows one call can re-evaluate.  A call whose candidate rows      */
                                /*     exceed it re-evaluates NONE: every ambiguous pair of the call keeps its fp32 answer (reproducible,    */
                                /*     the same on every rank of a sharded merge -- which pairs would have found room is not) and is         */
                                /*     counted in gacq_get_tie_stats()[2].  The automatic capacity is bounded (never below                  */
                                /*     16) so that the re-evaluation's row buffers (B x N x 8-24 bytes per listed row, allocated for the    */
                                /*     capacity) stay within an eighth of the workspace limit (gacq_set_workspace_limit), between 32 and    */
                                /*     256 MiB; an explicit value is taken as given                                                         */
#define GACQ_OPT_FUSED_C128 16     /* [1] engine 5 on the hand-written complex128 kernels where they exist -- N = 4096, B = 1, one carrier: the     */
                                /*     whole search row in one workgroup; N = 16384 / 65536: the split form (c128_split_*_kernel); N = 61380 /    */
                                /*     30690: the 31 x M form (c128_r31_*_kernel) -- instead of the five-stage rocFFT double-precision pipeline; */
                                /*     0 = always the pipeline (the cross-check)                                                                */
#define GACQ_OPT_SPLIT_MFMA 17     /* [0] prime-factor engine: the inverse DFT-31 of the outer stage as two real 16 x 16 matrices on the       */
                                /*     matrix pipe (v_mfma_f32_16x16x4_f32, exact fp32) instead of packed math on the VALU.  Off: measured     */
                                /*     12-18 % slower -- the stage is paced by its load stream, not by arithmetic                             */
                                /*     (profiles/r05_engine3_prime_factor_vs_cooley_tukey_ab.log)                                             */
#define GACQ_OPT_F4K_RUN 18        /* [1] takes effect only where claimed work (GACQ_OPT_F4K_CLAIM) is off or not engaged -- with the defaults a    */
                                /*     batch large enough for claimed work ignores it, so a sweep of it sets GACQ_OPT_F4K_CLAIM = 0 too.     */
                                /*     Fused N = 4096 kernel, static map: consecutive work items (epoch, Doppler bin, item chunk) one       */
                                /*     workgroup walks, paying its set-up once; 1 = one work item per workgroup; 0 = the fewest runs that   */
                                /*     leave four rounds of resident workgroups (16 per compute unit); always capped at the work items of   */
                                /*     one epoch.  Runs longer than 1 measured slower (profiles/r17_fused4k_unit_runs_ab.log): what they save in    */
                                /*     set-up they lose at the end of the launch, where slots wait for the slowest                          */
#define GACQ_OPT_F4K_CLAIM 19      /* [1] fused N = 4096 kernel: 1 = claimed work when there is more work than resident workgroups: one workgroup  */
                                /*     per resident slot (4 per compute unit) stays for the whole launch and takes work items from eight    */
                                /*     queues (one per XCD, atomic counters), from another XCD's queue when its own is empty; 0 = the static */
                                /*     map of GACQ_OPT_F4K_RUN; n > 1 = claimed work with n workgroups whatever the shape (tests, sweeps)    */
#define GACQ_NOPTS 20
int gacq_set_option(gacq_ctx* ctx, int option, long value);
int gacq_get_option(gacq_ctx* ctx, int option, long* value);

/* Build a signal: replicas from the built-in generators -> code spectra C_p resident on the device.
 * Replaces acquire-gps-l1.py:22-24 (c = ca.code(...); c = fft.fft(c)) for every PRN in `prns`. */
int gacq_signal_create(gacq_ctx* ctx, const gacq_sigdesc* desc, const char* code,
                       const int* prns, int nprn, gacq_sig** out);
/* Same, caller supplies the chips ({0,1} bytes, nprn rows of desc->code_length). */
int gacq_signal_create_chips(gacq_ctx* ctx, const gacq_sigdesc* desc, const uint8_t* chips,
                             int nprn, gacq_sig** out);
void gacq_signal_destroy(gacq_sig* sig);
int gacq_signal_fft_length(const gacq_sig* sig);        /* N = n or 2n */
/* Copy the device code spectrum of item `item` back (interleaved complex64, N values). Test hook. */
int gacq_signal_spectrum(gacq_sig* sig, int item, float* out_iq);

/* One search() per item over the same samples (host buffers, synchronous).
 *   x_iq      interleaved complex64, nsamp complex samples at desc->fs; needs (blocks+pad)*n
 *   items     indices into the signal's PRN list (0-based), nitems of them
 *   dopplers  the Doppler grid values np.arange(min,max,incr) produced (acquire-gps-l1.py:26)
 *   item_bias_hz  NULL, or per-item carrier bias added to the Doppler before the NCO
 *                 (GLONASS FDMA: 562500*chan, acquire-glonass-l1.py:28)
 *   blocks    number of non-coherent blocks B (the per-signal ms->B rule stays in the caller)
 * Replaces acquire-gps-l1.py:25-40 for all items at once (and the mp.Pool.map at :105-108).
 * Completion: the call returns when all `nitems` results are in `out`.  For small inputs on large-BAR devices (options
 * GACQ_OPT_BAR_UPLOAD / GACQ_OPT_WATCH_RESULTS, both on by default) it learns that by watching the pinned result records the last
 * kernel writes (bounded: 200 us, then hipStreamSynchronize, which is also where a faulted launch is reported) and does NOT
 * synchronise the ctx stream: trailing empty launches (the tie-safe re-evaluation kernels of a search without near-ties) may still
 * be queued when it returns.  They touch library-owned memory only; any later call on the ctx is ordered behind them. */
int gacq_search(gacq_sig* sig, const float* x_iq, size_t nsamp, const int* items, int nitems,
                const double* dopplers, int nd, const double* item_bias_hz, int blocks,
                gacq_result* out);

/* Batched, device-resident form: nepoch independent sample blocks already in HBM, results left in
 * HBM; asynchronous on the ctx stream.  d_x: complex64 [nepoch][nsamp]; d_out: gacq_peak
 * [nepoch][nitems] holding the best over `dopplers` (a rank's slice of the grid when sharded). */
int gacq_search_batch_dev(gacq_sig* sig, const void* d_x, size_t nsamp, int nepoch,
                          const int* items, int nitems, const double* dopplers, int nd,
                          const double* item_bias_hz, int blocks, void* d_out);

/* The same two entry points for complex128 samples -- the type the reference's search() is actually handed (np.interp's output,
 * acquire-gps-l1.py:94-96, used at :30-33).  x_iq / d_x_c128: interleaved (re, im) doubles.  Nothing is rounded where it matters:
 * engine 5 reads the samples as given; the fp32 engines search a complex64 rounding of them (made on the device) and every
 * (epoch, item) whose winner has a runner-up within GACQ_OPT_TIE_EPS_PPB -- which covers the rounding of the input, ~1e-7 -- is
 * re-evaluated in complex128 FROM THE UNROUNDED SAMPLES (tie-safe locations), so peak locations are those of the reference on its
 * own input and metrics agree within the 1e-5 of the fp32 engines.  gacq_search64 is synchronous (staged H2D copy, no BAR path). */
int gacq_search64(gacq_sig* sig, const double* x_iq, size_t nsamp, const int* items, int nitems,
                  const double* dopplers, int nd, const double* item_bias_hz, int blocks,
                  gacq_result* out);
int gacq_search_batch_dev64(gacq_sig* sig, const void* d_x_c128, size_t nsamp, int nepoch,
                            const int* items, int nitems, const double* dopplers, int nd,
                            const double* item_bias_hz, int blocks, void* d_out);

/* Host-buffer batch: nepoch independent sample blocks in HOST memory (x_iq: complex64 [nepoch][nsamp]) -> out [nepoch][nitems]
 * on the host.  Synchronous for the caller, pipelined inside: the epochs go through a ring of pinned staging slots in chunks,
 * the H2D copy of chunk c+1 runs on a copy stream under the kernels of chunk c, and the peak records are written by the last
 * kernel into device-visible pinned memory (no D2H copy).  Amortises the launch latency of gacq_search over many epochs for
 * callers without a device-memory framework; results are identical to nepoch calls of gacq_search. */
int gacq_search_batch(gacq_sig* sig, const float* x_iq, size_t nsamp, int nepoch, const int* items, int nitems,
                      const double* dopplers, int nd, const double* item_bias_hz, int blocks, gacq_result* out);

/* ---------------------------------------------------------------------------------------------
 * Several GPUs driven from ONE process (no torch, no MPI): a group owns one context per device.  gacq_group_search_batch cuts
 * the Doppler grid into contiguous slices, one per device, while every device still gets >= 4 bins (forward FFTs are not
 * duplicated; every device holds all code spectra), otherwise the item list; all devices read the same samples from one
 * portable pinned staging buffer; the per-device peak records (16 B per epoch and item) come back through pinned host memory
 * and are merged in global Doppler order with strict '>' -- the scan order of acquire-gps-l1.py:36-39, so the result equals
 * a one-device search bit for bit.  device_ids may name a device more than once.  Replaces the mp.Pool.map over PRNs
 * (acquire-gps-l1.py:105-108) for a single-process caller; one-process-per-GPU callers use torch.distributed (sharded.py).
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_group gacq_group;
typedef struct gacq_gsig gacq_gsig;
int gacq_group_create(const int* device_ids, int ndev, gacq_group** out);
void gacq_group_destroy(gacq_group* group);
int gacq_group_size(const gacq_group* group);
gacq_ctx* gacq_group_member(gacq_group* group, int k);   /* member context, e.g. for gacq_set_engine / gacq_set_option */
/* How the members' peak records meet.  GACQ_EXCHANGE_HOST [default]: each member's last kernel writes its records into pinned host
 * memory and the host merges them (near-ties re-evaluated on a member).  GACQ_EXCHANGE_RCCL: the records stay on the devices, ONE
 * ncclAllGather per chunk moves them over xGMI (single-process communicators from ncclCommInitAll; librccl.so is loaded on this
 * call, the library does not link against it) and a member merges them on the device with the tie-safe merge -- the same result bit
 * for bit.  Needs distinct devices; GACQ_ERR_UNSUPPORTED otherwise or when RCCL cannot be loaded (the group then stays on the host
 * merge).  Applies to Doppler-sliced searches; an item split needs no merge.  EXPERIMENTAL beyond one device: the mode has run on one
 * MI355X (a one-rank collective) and never on several -- no multi-GPU node was available to rounds 1-6.  A failed collective aborts the
 * communicators (ncclCommAbort: nothing stays queued on a member's stream), returns the group to GACQ_EXCHANGE_HOST and reports the
 * error; the call can be repeated. */
#define GACQ_EXCHANGE_HOST 0
#define GACQ_EXCHANGE_RCCL 1
int gacq_group_set_exchange(gacq_group* group, int mode);
const char* gacq_group_last_error(gacq_group* group);
int gacq_group_signal_create(gacq_group* group, const gacq_sigdesc* desc, const char* code, const int* prns, int nprn,
                             gacq_gsig** out);
void gacq_group_signal_destroy(gacq_gsig* sig);
int gacq_group_search_batch(gacq_gsig* sig, const float* x_iq, size_t nsamp, int nepoch, const int* items, int nitems,
                            const double* dopplers, int nd, const double* item_bias_hz, int blocks, gacq_result* out);

/* Tie-safe bookkeeping since gacq_create (synchronises the ctx stream): out[0] ambiguous (epoch, item) pairs found, out[1] rows
 * re-evaluated in complex128, out[2] pairs that kept their fp32 answer because the re-evaluation list was full (GACQ_OPT_TIE_CAP and its
 * memory bound) -- anything but 0 here means locations that are NOT guaranteed to be the complex128 ones: treat it as a warning
 * (bench.py prints one), out[3] pairs whose location the re-evaluation changed.  FFT lengths with a prime factor the complex128 row kernel
 * does not carry (it has 2, 3, 5, 7, 11, 13 and 31: every length the reference's scripts use) are searched without tie-safe locations
 * and are not counted here. */
int gacq_get_tie_stats(gacq_ctx* ctx, long long out[4]);

/* Device-side shard merge: d_peaks [nshard][n] (as gathered from the ranks, shard s covering Doppler
 * indices from shard_d0[s]) -> d_out [n] with global d_index; shards scanned in order with strict '>'
 * so the lowest Doppler bin wins ties exactly like the reference's scan (acquire-gps-l1.py:36-39).
 * Asynchronous on the ctx stream. */
int gacq_merge_peaks_dev(gacq_ctx* ctx, const void* d_peaks, int nshard, const int* shard_d0, long n,
                         void* d_out);

/* The same merge for callers that run with tie-safe locations (GACQ_OPT_TIE_SAFE, the default): shard winners whose metrics come
 * within GACQ_OPT_TIE_EPS_PPB of the best one are re-evaluated in complex128 on this device before the scan decides -- every rank
 * holds the samples and all code spectra, so any rank can do it -- which makes the merged record the one an unsharded tie-safe
 * search writes, bit for bit.  The search arguments are those of the search the shards came from, with the FULL Doppler grid
 * (d_x: [nepoch][nsamp] on the device).  Asynchronous on the ctx stream. */
int gacq_merge_peaks_tiesafe_dev(gacq_sig* sig, const void* d_x, size_t nsamp, int nepoch, const int* items, int nitems,
                                 const double* dopplers, int nd, const double* item_bias_hz, int blocks, const void* d_peaks,
                                 int nshard, const int* shard_d0, void* d_out);
/* ... with the samples in complex128 (see gacq_search_batch_dev64) */
int gacq_merge_peaks_tiesafe_dev64(gacq_sig* sig, const void* d_x_c128, size_t nsamp, int nepoch, const int* items, int nitems,
                                 const double* dopplers, int nd, const double* item_bias_hz, int blocks, const void* d_peaks,
                                 int nshard, const int* shard_d0, void* d_out);

/* Host-side last step (acquire-gps-l1.py:36-40): merge `nshard` peaks per item in shard order with
 * strict '>' (shard s covers Doppler indices [shard_d0[s], ...)), then convert to the reference's
 * return tuple.  peaks: [nshard][nitems]; dopplers: the FULL grid.  Needs no GPU. */
int gacq_finalize(const gacq_sigdesc* desc, const gacq_peak* peaks, int nshard, const int* shard_d0,
                  int nitems, const double* dopplers, int nd, gacq_result* out);

/* ---------------------------------------------------------------------------------------------
 * Front-end (SURVEY.md section 8f "next #1"): what every acquire script does to the file before search().
 * Replaces acquire-gps-l1.py:87-96: nco.mix (fixed-point table NCO, gnsstools/nco.py:30-41),
 * scipy.signal.filtfilt(h,[1],x) with a firwin(161, cutoff, 'hann') low-pass, np.interp resample.
 * ------------------------------------------------------------------------------------------- */
/* scipy.signal.firwin(ntaps, cutoff_norm, window='hann'); cutoff_norm = cutoff_hz / (fs/2). Host only. */
int gacq_firwin_hann(int ntaps, double cutoff_norm, double* taps);
/* d_iq_int8: interleaved signed 8-bit I/Q on the device (nsamp_in complex samples at fs_in);
 * d_out: complex64 [nsamp_out] at fs_out, directly consumable by gacq_search_batch_dev. Asynchronous. */
int gacq_frontend_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nsamp_in, double fs_in, double carrier_offset_hz,
                      const double* taps, int ntaps, double fs_out, size_t nsamp_out, void* d_out);

/* The main program of an acquire script in one call (acquire-gps-l1.py:78-108: read block, mix / filter / resample, search every item):
 * iq_int8 = nsamp_in interleaved signed 8-bit I/Q samples at fs_in in HOST memory; the block is uploaded, gacq_frontend_dev produces
 * nsamp_out samples at the signal's internal rate on the device and gacq_search_batch_dev searches them there; out[nitems] as
 * gacq_search.  For callers without a device-memory framework (the command-line shim runs on it: no torch import on its path).
 * Synchronous; GACQ_WARN_TIE_LIST_FULL as gacq_search. */
int gacq_acquire_int8(gacq_sig* sig, const int8_t* iq_int8, size_t nsamp_in, double fs_in, double carrier_offset_hz, const double* taps,
                      int ntaps, size_t nsamp_out, const int* items, int nitems, const double* dopplers, int nd,
                      const double* item_bias_hz, int blocks, gacq_result* out);

/* The front-end for many windows of one recording at once: window w is the nsamp_in samples that begin at sample starts[w] of
 * d_iq_int8 (interleaved signed 8-bit I/Q on the device, nsamp_avail complex samples; any start is allowed, windows may overlap or
 * leave gaps), and row w of d_out (complex64 [nwin][nsamp_out]) is, bit for bit, what gacq_frontend_dev writes for that slice: the
 * mixer phase restarts at 0 and filtfilt extends every window on its own.  One launch set serves all windows of a chunk; a chunk is
 * as many windows as the workspace limit allows intermediates, and the result does not depend on the chunking.  For the 161-tap
 * filter the backward pass and the resampler are one kernel that computes only the two filtered samples each output reads.
 * starts: HOST array, int64, staged by the call (it may be reused on return).  GACQ_ERR_SHORT_INPUT when nsamp_in <= 3*ntaps or a
 * window does not lie inside [0, nsamp_avail); refusals are made before anything is allocated or launched.  Asynchronous. */
int gacq_frontend_batch_dev(gacq_ctx* ctx, const void* d_iq_int8, long long nsamp_avail, const long long* starts, int nwin,
                            size_t nsamp_in, double fs_in, double carrier_offset_hz, const double* taps, int ntaps, double fs_out,
                            size_t nsamp_out, void* d_out);

/* gacq_acquire_int8 at many positions of a recording that is already on the device (scan.py): gacq_frontend_batch_dev into a
 * library-owned buffer, then ONE gacq_search_batch_dev with the windows as its epochs, per chunk of windows that fits the workspace
 * limit.  d_peaks: gacq_peak [nwin][nitems], device or device-visible pinned memory; gacq_finalize turns a row into the results
 * gacq_acquire_int8 returns for that window (locations equal, tie-safe; metrics within the 1e-5 of the fp32 engines, because a
 * batch may take another kernel form than a single epoch).  Argument checks as gacq_acquire_int8 and gacq_frontend_batch_dev, all
 * made before anything is launched.  Asynchronous, so unlike gacq_acquire_int8 it cannot return GACQ_WARN_TIE_LIST_FULL: a caller
 * that needs to know reads gacq_get_tie_stats()[2] after the call.  Memory: the library-owned buffer of front-end output, the
 * front-end's intermediates and the search's two workspaces are each sized from the workspace limit on their own, so the call can
 * hold up to four times that limit (less whenever the windows need less). */
int gacq_scan_int8_dev(gacq_sig* sig, const void* d_iq_int8, long long nsamp_avail, const long long* starts, int nwin, size_t nsamp_in,
                       double fs_in, double carrier_offset_hz, const double* taps, int ntaps, size_t nsamp_out, const int* items,
                       int nitems, const double* dopplers, int nd, const double* item_bias_hz, int blocks, void* d_peaks);

/* ---------------------------------------------------------------------------------------------
 * Time-domain long-code searches (SURVEY.md section 8f "next #3"): acquire-gps-l2cl.py:15-30,
 * acquire-glonass-l1-p.py / -l2-p.py:15-33.  For candidate k:
 *   q[k] = sum_block | sum_i x[n*block+i] * code[floor(phase0[k*blocks+block] + (chip_rate/fs)*i) mod L] * nco[i] |
 * x_iq: host complex64 at the file rate fs (after the carrier-offset wipe-off); carrier_hz = Doppler (+ FDMA channel bias);
 * phase0: the caller's (chips % L) + frac per (k, block), in chips -- finite and within +-2^31 chips (anything else is
 * GACQ_ERR_BAD_ARG; the reference's expressions stay below two code periods).  Synchronous; q_out[K] in fp64.
 * ------------------------------------------------------------------------------------------- */
int gacq_longcode_search(gacq_ctx* ctx, const float* x_iq, size_t nsamp, double fs, const char* code, int prn,
                         double carrier_hz, const double* phase0, int K, int blocks, int n, double* q_out);
/* Same from the file's raw samples: iq_int8 = interleaved signed 8-bit I/Q (host, nsamp complex samples, gnsstools/io.py:3-12);
 * the carrier-offset wipe-off nco.mix(x,-coffset/fs,0) (acquire-gps-l2cl.py:72, fixed-point table NCO of gnsstools/nco.py:30-41)
 * runs on the device before the search, so the caller does no per-sample work at all. */
int gacq_longcode_search_int8(gacq_ctx* ctx, const int8_t* iq_int8, size_t nsamp, double fs, double carrier_offset_hz,
                              const char* code, int prn, double carrier_hz, const double* phase0, int K, int blocks, int n,
                              double* q_out);

/* ---------------------------------------------------------------------------------------------
 * Batched code correlators for the tracking hand-off (SURVEY.md section 8f "next #4"): the reference's
 * <module>.correlate(x, prn, chips, frac, incr, c[, boc11]) (gnsstools/gps/ca.py:120-128 and its BOC / CBOC / TMBOC /
 * RZ variants) for K (PRN, start phase, rate) triples over one block of n samples in one launch.
 * kind: 0 plain, 1 BOC(1,1), 2 CBOC (e1b/e1c), 3 TMBOC (l1cp), 4 RZ first half chip (l2cm), 5 RZ second half (l2cl).
 * out_iq: K interleaved complex128 sums.  Synchronous; x_iq is a host buffer.
 * ------------------------------------------------------------------------------------------- */
int gacq_correlate_batch(gacq_ctx* ctx, const float* x_iq, size_t n, const char* code, int kind, const int* prns,
                         const double* chips, const double* frac, const double* incr, int K, double* out_iq);

/* Device-resident forms of the two entry points above: d_x is complex64 ALREADY on the device (gacq_frontend_dev's or
 * gacq_mix_int8_dev's output, or the very samples gacq_search_batch_dev just searched) -- the reference keeps one x in memory from
 * acquisition into the long-code search (acquire-gps-l2cl.py:60-76) and into correlate() every millisecond
 * (track-gps-l1.py:48-50).  Only the start phases / the K correlator specs travel to the device; results come back through pinned
 * memory into q_out / out_iq.  Same kernels, byte-identical results. */
int gacq_longcode_search_dev(gacq_ctx* ctx, const void* d_x, size_t nsamp, double fs, const char* code, int prn, double carrier_hz,
                             const double* phase0, int K, int blocks, int n, double* q_out);
int gacq_correlate_batch_dev(gacq_ctx* ctx, const void* d_x, size_t n, const char* code, int kind, const int* prns,
                             const double* chips, const double* frac, const double* incr, int K, double* out_iq);
/* nco.mix(x, -coffset/fs, 0) alone on the device (gnsstools/nco.py:30-41; acquire-gps-l2cl.py:72): d_iq_int8 interleaved signed 8-bit
 * I/Q -> d_out complex64 [nsamp] at the same rate.  Asynchronous on the ctx stream. */
int gacq_mix_int8_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nsamp, double fs, double carrier_offset_hz, void* d_out);

/* ---------------------------------------------------------------------------------------------
 * The reference's signal-inspection utilities on the device (gacq_spectrum.hip).  Both are asynchronous on the ctx stream; bad
 * arguments return GACQ_ERR_BAD_ARG before anything is launched.
 * ------------------------------------------------------------------------------------------- */
/* Welch power spectrum (spectrum.py:48-57): d_iq_int8 holds nspectra * ns consecutive frames of n interleaved signed 8-bit I/Q samples;
 * per frame int8 -> float, times d_window (float[n], np.hanning(n) rounded to fp32), complex64 FFT of length n in LDS, re^2 + im^2;
 * the ns frames of a spectrum are accumulated in fp64, divided by ns, fftshift-ed and written as 10 log10 to d_out_db (double
 * [nspectra][n]; a bin of power 0 gives -inf).  n: a power of two from 64 to 16384.  split: workgroups per spectrum (0: chosen from
 * nspectra); the output bits do not depend on it.  d_iq_int8 and d_window must be 16-byte aligned. */
int gacq_psd_int8_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nspectra, int n, int ns, const void* d_window, int split, void* d_out_db);
/* Squaring-loop carrier detector (squaring.py:28-40, gnsstools/squaring.py:14-23, gnsstools/nco.py:30-41): d_iq_int8 holds nchunks
 * chunks of `chunk` = b*n*m samples.  Sample i of chunk c is multiplied by the table NCO at the 64-bit wrapping phase
 * floor(d_phase0[c] * 2^60) + i * floor(f * 2^60) (f = -coffset/fs; d_phase0: double[nchunks] on the device, the script's
 * coffset_phase at each chunk's start), the product rounded to complex64; n consecutive products are summed in fp64 to s, m values of
 * s*s/n are summed to one output.  d_r: complex128 [nchunks][b]; d_y: the script's int16 stream, round-half-even of 20 re, 20 im
 * interleaved and clamped to the int16 range; d_clamped: one uint64, the number of clamped values. */
int gacq_squaring_int8_dev(gacq_ctx* ctx, const void* d_iq_int8, size_t nchunks, size_t chunk, int n, int m, const void* d_phase0, double f,
                           void* d_r, void* d_y, void* d_clamped);

/* ---------------------------------------------------------------------------------------------
 * Device-resident tracking loops: the template family of the reference's track-*.py (track-gps-l1.py:33-179 and the scripts that
 * differ from it only in the constants below), one workgroup per channel walking its own blocks -- offset and carrier wipe-off
 * (table NCO), early/prompt/late, FLL/PLL/DLL update -- with the state kept on the device between calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_track gacq_track;

typedef struct gacq_track_spec {   /* one channel: the script's constants and its command line */
  const char* code;                /* code module, e.g. "gps.ca" */
  int prn;                         /* PRN (GLONASS: 0) */
  int kind;                        /* correlator kind of gacq_correlate_batch (0 plain .. 5 RZ [0,1]) */
  int subs;                        /* track() calls per outer block: 1, 4, 10 or 20 */
  int fixed_pll;                   /* 1: mode is PLL from the start and never switches (Xona) */
  int glonass;                     /* 1: offset phase advances by n*fm (fm = -(coffset + step*chan)/fs), else by -(n*coffset)/fs */
  int pad;
  double fs;                       /* sample rate, Hz */
  double period;                   /* seconds per outer block (0.001, 0.004, 0.01, 0.020) */
  double rate;                     /* its inverse as the script writes it (1000.0, 250.0, 100.0, 50.0) */
  double ratio;                    /* carrier / code frequency ratio of cf = (code_f + carrier_f/ratio)/fs */
  double spacing;                  /* early/late offset, chips */
  double chip_rate;                /* initial code_f */
  double fll_k_wide, fll_k_narrow, pll_k1, pll_k2, dll_k1, dll_k2;
  double coffset;                  /* carrier_offset argument, Hz */
  double fm;                       /* GLONASS: -(coffset + step*chan)/fs; otherwise unused */
  double code_offset;              /* code_offset argument, chips, in [0, L) */
  double doppler;                  /* doppler argument, Hz */
  double carrier_phase;            /* initial carrier phase, cycles */
  double dwell_wide, dwell_narrow; /* --loop-dwells, records (0, 0 with --carrier-phase) */
} gacq_track_spec;

typedef struct gacq_track_record { /* one track() call: what the script prints */
  double p_re, p_im, carrier_f, code_f, early, prompt, late, code_p, carrier_p;
  long long block, code_cyc, carrier_cyc, samp;
} gacq_track_record;

typedef struct gacq_track_chstate {  /* a channel's loop state between calls */
  double code_p, code_f, carrier_p, carrier_f, prompt1_re, prompt1_im, carrier_e1, code_e1, coffset_phase;
  long long pos;                   /* next block's first sample in the channel's recording */
  long long block, samp, code_cyc, carrier_cyc;
  int mode;                        /* 0 FLL_WIDE, 1 FLL_NARROW, 2 PLL (of the last record) */
  int status;                      /* GACQ_TRACK_* */
  int last_records;                /* records the last gacq_track_run_dev call wrote */
  int pad;
} gacq_track_chstate;

#define GACQ_TRACK_RUNNING 0
#define GACQ_TRACK_BAD_BLOCK 1    /* the block length came out NaN or below one sample: the channel stopped */
#define GACQ_TRACK_BAD_PHASE 2    /* an NCO phase or rate is not finite or out of the fixed-point range: the channel stopped */
#define GACQ_TRACK_BAD_WINDOW 3   /* long-code loops: a sub-block's code span does not fit the LDS chip window: the channel stopped */

/* K channels; every spec is checked before anything is allocated, and the code-boundary alignment of the script is done here. */
int gacq_track_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, gacq_track** out);
/* One launch on the ctx stream: channel k's samples d_x[k] (device, interleaved int8 I/Q) are samples [base[k], base[k] + avail[k])
 * of its recording; each channel writes at most max_records records (whole outer blocks; a record is one track() call, 1 ms of
 * signal), stopping at the first block those samples cannot fill.  base[k] must not lie beyond the channel's next block.
 * records: [K][rec_cap] (subs <= max_records <= rec_cap), counts[K] records written, status[K] GACQ_TRACK_*.  Synchronous. */
int gacq_track_run_dev(gacq_track* tr, const void* const* d_x, const long long* base, const long long* avail, int max_records,
                       gacq_track_record* records, int rec_cap, int* counts, int* status);
int gacq_track_state(gacq_track* tr, int k, gacq_track_chstate* out);
void gacq_track_close(gacq_track* tr);
/* ---------------------------------------------------------------------------------------------
 * Device-resident tracking loops for the long-code scripts: track-gps-l2cl.py (1500 track() calls per 1.5 s outer block) and
 * track-glonass-l1-p.py / -l2-p.py (1000 per 1 s).  Same specs, records and states as gacq_track_*, and the same arithmetic; the code
 * table stays in device memory and each sub-block reads a window of it.  kind 0 or 4 / 5 (RZ), subs <= 1500, any code length.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_longtrack gacq_longtrack;

int gacq_longtrack_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, gacq_longtrack** out);
/* As gacq_track_run_dev: whole outer blocks only (subs <= max_records <= rec_cap), status GACQ_TRACK_* (BAD_WINDOW included). */
int gacq_longtrack_run_dev(gacq_longtrack* tr, const void* const* d_x, const long long* base, const long long* avail, int max_records,
                           gacq_track_record* records, int rec_cap, int* counts, int* status);
int gacq_longtrack_state(gacq_longtrack* tr, int k, gacq_track_chstate* out);
void gacq_longtrack_close(gacq_longtrack* tr);

/* ---------------------------------------------------------------------------------------------
 * Tracking loops with the chip accumulator: track-beidou-b2bi.py / -b2bq.py.  The template loop of gacq_track_* (same specs, records,
 * states and arithmetic) plus, for every track() call whose frame number (the record's block) exceeds accum_after[k], the script's
 * nco.accum(+-x, code_p, cf, chips, L): each wiped-off complex64 sample is added to bin floor(code_p + cf*i) mod L of a complex128
 * accumulator, negated when real(p_prompt) <= 0; every bin is the sequential fp64 sum in sample order, across blocks and launches.
 * kind 0 and L <= 10240 only.  Accumulator and state persist between gacq_chiptrack_run_dev calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_chiptrack gacq_chiptrack;

int gacq_chiptrack_open(gacq_ctx* ctx, const gacq_track_spec* specs, int K, const long long* accum_after, gacq_chiptrack** out);
/* As gacq_track_run_dev. */
int gacq_chiptrack_run_dev(gacq_chiptrack* tr, const void* const* d_x, const long long* base, const long long* avail, int max_records,
                           gacq_track_record* records, int rec_cap, int* counts, int* status);
int gacq_chiptrack_state(gacq_chiptrack* tr, int k, gacq_track_chstate* out);
/* Channel k's accumulator: 2 L doubles, re / im interleaved.  Synchronous. */
int gacq_chiptrack_chips(gacq_chiptrack* tr, int k, double* out);
void gacq_chiptrack_close(gacq_chiptrack* tr);

/* The loop's two wipe-offs alone, for checking them bit for bit: d_out[k] (complex64) = nco.mix(nco.mix(x, f_offset, p_offset),
 * f_carrier, p_carrier)[k] for the n int8 I/Q samples at d_iq_int8, computed by the loop's own device helpers.  Synchronous. */
int gacq_track_debug_mix(gacq_ctx* ctx, const void* d_iq_int8, size_t n, double f_offset, double p_offset, double f_carrier,
                         double p_carrier, void* d_out);

/* ---------------------------------------------------------------------------------------------
 * Correlation grid on the raw recording (gacq_corrgrid.hip): the fine search between acquisition and tracking.  For K candidates in
 * one launch, the prompt correlation over M blocks of n samples, D Doppler hypotheses and P code-phase hypotheses.  With
 * j = s0 + m n + i the absolute sample index of the candidate's recording,
 *     f_d = doppler0 + (d - (D-1)/2) df,   cf = (chip_rate + doppler0/ratio) / fs,
 *     C[k,m,d,p] = sum_{i<n} x[j] exp(-2 pi i frac((carrier_hz + f_d) j / fs)) w(code0 + offsets[p] + cf j)
 * with w the chip weight of the tracking loops' correlator `kind` (subcarrier phases 2 pos and 12 pos of the same start phase).  The
 * exponential is the exact one (64-bit phase reduction, no table NCO); the sums are fp32 per lane, fp64 across waves.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_grid_spec {
  const char* code;                /* code module, e.g. "gps.ca" */
  int prn;                         /* PRN (GLONASS: 0) */
  int kind;                        /* correlator kind of gacq_correlate_batch (0 plain .. 5 RZ [0,1]) */
  int n;                           /* samples per block, >= 1 */
  int M;                           /* blocks, >= 1 */
  int D;                           /* Doppler hypotheses, 1..33 */
  int P;                           /* code-phase hypotheses, 1..33 */
  double fs;                       /* sample rate of the recording, Hz */
  double carrier_hz;               /* carrier offset wiped off with every hypothesis (GLONASS: coffset + step * chan) */
  double chip_rate;                /* nominal chip rate, chips/s */
  double ratio;                    /* carrier / code frequency ratio; the code rate uses doppler0 for every hypothesis */
  double doppler0;                 /* centre of the Doppler axis, Hz */
  double code0;                    /* code phase at sample 0 of the recording, chips */
  double df;                       /* Doppler step, Hz */
  long long s0;                    /* first sample of block 0 */
  const double* offsets;           /* P code offsets in chips, relative to code0 (host memory) */
} gacq_grid_spec;

/* d_x[k]: candidate k's recording on the device, interleaved signed 8-bit I/Q, avail[k] complex samples (candidates may share one);
 * nothing outside [0, 2 avail[k]) bytes is read.  out (host): complex128, candidate after candidate, each [M][D][P] -- [K][M][D][P]
 * when the candidates share M, D and P.  Every argument is checked before anything is launched: s0 + M n > avail returns
 * GACQ_ERR_SHORT_INPUT; n, M < 1, D or P outside 1..33, a value that is not finite, ratio = 0 GACQ_ERR_BAD_ARG; an unknown code or
 * PRN GACQ_ERR_UNKNOWN_CODE / GACQ_ERR_BAD_PRN; a code longer than 10240 chips GACQ_ERR_UNSUPPORTED.  One launch on the ctx stream,
 * one workgroup per (candidate, block); a result's bits depend only on its own candidate and block.  Synchronous. */
int gacq_corr_grid_dev(gacq_ctx* ctx, const gacq_grid_spec* specs, int K, const void* const* d_x, const long long* avail, double* out);

/* ---------------------------------------------------------------------------------------------
 * Coherent fold ahead of the search (gacq_cohfold.hip): M code periods summed under H sign hypotheses, per Doppler value, so that the
 * search of a folded row is the coherent search over M periods (correlation is linear).  With x complex64 on the device (wide != 0:
 * complex128, rounded once), j0 the absolute sample index of x[0], D Doppler values f_d (Hz), H patterns W[h][m] in {-1, 0, +1} and
 * a start table start[d][m] in samples of x (both row-major, host memory),
 *     y[d,h,i] = sum_{m<M} W[h,m] x[start[d,m] + i] exp(-2 pi i frac(f_d (j0 + start[d,m] + i) / fs)),   0 <= i < n_out.
 * d_y: complex64 [D][H][n_out] on the device, contiguous.  The exponential is exact per sample (64-bit fixed-point phase reduced
 * before it becomes fp32; no table NCO, nothing extrapolated along the Doppler axis); the sum is fp32 in the order of m.  The bits of
 * y[d,h,:] depend on row d's inputs and on W[h] alone -- not on D, H, or how a caller splits the rows over calls.
 * Every argument is checked before anything is allocated or launched: n_out, M, D or H < 1, M > 128, H > 256, f_d or fs not finite,
 * fs <= 0, a W entry outside -1..1, |j0| > 2^62 GACQ_ERR_BAD_ARG; start[d][m] < 0 or start[d][m] + n_out > avail (complex samples at
 * d_x) GACQ_ERR_SHORT_INPUT.  One launch on the ctx stream; asynchronous.
 * ------------------------------------------------------------------------------------------- */
int gacq_fold_dev(gacq_ctx* ctx, const void* d_x, int wide, long long avail, int n_out, int M, int D, int H, const long long* start,
                  const double* f_d, double fs, long long j0, const signed char* W, void* d_y);

/* ---------------------------------------------------------------------------------------------
 * Synthetic recordings (gacq_simulate.hip): samples j = j0 .. j0 + n - 1 of one endless recording of K satellites plus white noise,
 * an exact function of (scene, seed, absolute sample index j) -- the same bytes however a caller cuts it into calls:
 *     v(j) = noise(j) + sum_{k<K} amp_k w_k(j) d_k(j) exp(2 pi i theta_k(j) / 2^64),       noise first, then k ascending, in fp32.
 * Per satellite, converted once from the doubles below in IEEE double operations:
 *     F = floor(frac(carrier_hz / fs) 2^64), p0 likewise from carrier_phase (turns); theta(j) = (p0 + j F) mod 2^64.  The frequency
 *       produced differs from the request by less than fs 2^-53.
 *     Cf = floor((code_rate_hz / fs) 2^64), c0 likewise from code_phase (chips at j = 0); pos(j) = c0 + j Cf, an exact integer:
 *       chip index (pos >> 64) mod L, period (pos >> 64) div L, subchip fraction pos mod 2^64.
 *     w: the chip weight of correlator kind 0..5 (plain, BOC(1,1), CBOC 0.953463 / 0.301511, TMBOC, RZ [1,0], RZ [0,1]) with the
 *       half-chip bit = top bit of the fraction and the BOC(6,1) bit = floor(12 fraction / 2^64) mod 2.
 *     d = symbols[(period div periods_per_symbol) mod nsym], +1 when nsym = 0.
 * noise: Philox4x32-10, key (seed lo32, seed hi32), counter (j lo32, j hi32, 0, 0), words r0, r1;
 *     u1 = ((r0 >> 8) + 0.5) 2^-24, u2 = ((r1 >> 8) + 0.5) 2^-24, (nI, nQ) = sigma sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2).
 * d_out (device): complex64 [n] (out_complex64 != 0, 8-byte aligned), or interleaved signed 8-bit I/Q [2 n] = clip(rint(v), -127, 127)
 * with ties to even, of the very values the complex64 form holds.
 * Every argument is checked before anything is allocated or launched: K outside 1..32, n < 1, j0 < 0, j0 + n > 2^48, a value that is
 * not finite, fs <= 0, sigma < 0, code_rate_hz <= 0 or code_rate_hz / fs >= 16, code_phase outside [0, L), kind outside 0..5, nsym < 0
 * or > 2^20, a symbol other than +-1, periods_per_symbol < 1, a NULL pointer GACQ_ERR_BAD_ARG; an unknown code or PRN
 * GACQ_ERR_UNKNOWN_CODE / GACQ_ERR_BAD_PRN.  Chip tables are the context's cached ones (shared with the tracking loops), generated on
 * first use.  One launch on the ctx stream, no state kept; asynchronous.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_sim_sat {
  const char* code;                /* code module, e.g. "gps.ca" */
  int prn;                         /* PRN (GLONASS: 0) */
  int kind;                        /* chip weight, 0 plain .. 5 RZ [0,1] */
  int periods_per_symbol;          /* code periods per symbol, >= 1 */
  int nsym;                        /* symbols, 0..2^20; 0: every symbol is +1 */
  int pad;
  const int8_t* symbols;           /* nsym values +-1 (host memory); may be NULL when nsym = 0 */
  double amp;                      /* amplitude per component, LSB */
  double carrier_hz;               /* carrier frequency in the recording, Hz (offset + Doppler) */
  double carrier_phase;            /* carrier phase at j = 0, turns */
  double code_rate_hz;             /* chips per second */
  double code_phase;               /* code phase at j = 0, chips, in [0, L) */
} gacq_sim_sat;

int gacq_simulate_dev(gacq_ctx* ctx, const gacq_sim_sat* sats, int K, double fs, double sigma, unsigned long long seed, long long j0,
                      long long n, int out_complex64, void* d_out);

/* ---------------------------------------------------------------------------------------------
 * Array-and-interference scenes (gacq_scene.hip): samples j = j0 .. j0 + n - 1 of antennas a = first_antenna .. first_antenna + M - 1
 * of one endless multi-antenna recording, an exact function of (scene, seed, antenna, absolute sample index) -- the same bytes however
 * a caller cuts it into calls or into groups of antennas:
 *     v_a(j) = noise_a(j) + sum_{e < K + I} G[a][e] z_e(j),     noise first, then e ascending, in fp32: the K satellites, then the I
 *     emitters; per source  vr = fma(-Gi, zi, fma(Gr, zr, vr)),  vi = fma(Gi, zr, fma(Gr, zi, vi)).
 * Satellites, e < K: z_e(j) is the term amp w d exp(2 pi i theta / 2^64) of gacq_simulate_dev, from the same gacq_sim_sat by the same
 *     conversions, rounded to fp32 per component.  K = 0..32.
 * Antenna noise: gacq_simulate_dev's Box-Muller of Philox4x32-10, key = seed, counter (j lo32, j hi32, a, 0): antenna 0 has the
 *     stream of gacq_simulate_dev.  sigma is per component and the same for every antenna.
 * Emitters, i = e - K, I = 0..8, one gacq_scene_emitter each:
 *     gate: on(j) when gate_period = 0, else when ((j - gate_first) mod gate_period) < gate_on (the non-negative modulus), with
 *       0 <= gate_first < gate_period <= 2^48 and 1 <= gate_on <= gate_period.  z = 0 while the gate is off; the phase runs on.
 *     kind 0, tone: theta(j) = p0 + j F0 mod 2^64, F0 = floor(frac(f0_hz / fs) 2^64), p0 likewise from phase (turns at j = 0);
 *       z = amp exp(2 pi i theta / 2^64).
 *     kind 1 sawtooth chirp, kind 2 triangle chirp: the frequency word steps once per sample, W(u) = F0 + R ramp(u) mod 2^64 at
 *       u = j mod P (P = sweep), theta(j) = p0 + sum_{t<j} W(t mod P) mod 2^64.  Sawtooth: ramp(u) = u, R = floor((f1_hz - f0_hz) / fs
 *       / P 2^64).  Triangle: P even, H = P / 2, ramp(u) = u below H and P - 1 - u from H on, R = floor((f1_hz - f0_hz) / fs / H 2^64).
 *       R is a signed integer taken mod 2^64 (the two divisions in fp64, in that order; the scaling is exact).  Closed form:
 *       theta = p0 + s Phi + u F0 + R T(u), s = j div P, Phi = P F0 + R T(P), T(u) = u (u - 1) / 2 on the rising ramp (u <= H; the whole
 *       sawtooth) and H (H - 1) + (u - H)(P - 1) - u (u - 1) / 2 beyond; all products wrap mod 2^64.
 *     kind 3, broadband noise: Box-Muller of the same Philox with counter (j lo32, j hi32, i, 1) and amp as its sigma per component:
 *       one waveform common to all antennas, a point source.
 * gains (host): doubles [M][K + I][2] (re, im), each rounded once to fp32; row p belongs to antenna first_antenna + p.  The narrowband
 *     array model lives in these numbers only.
 * d_out (host array of M device pointers): each complex64 [n] (out_complex64 != 0, 8-byte aligned) or interleaved signed 8-bit I/Q
 *     [2 n] = clip(rint(v), -127, 127), ties to even, of the very values the complex64 form holds, at any address.
 * gacq_scene_check makes every check that needs no chip generator, before anything is allocated or launched: what gacq_simulate_dev
 *     refuses except K = 0; M outside 1..8; first_antenna outside 0 .. 2^31 - M; I outside 0..8; kind outside 0..3; a chirp sweep
 *     outside 2..2^31, an odd triangle sweep, |f1_hz - f0_hz| > fs; gate fields outside the ranges above; a value that is not finite (a
 *     gain: in fp32); a NULL pointer (sats with K = 0, emitters with I = 0 and gains with K + I = 0 may be NULL); a complex64 row that
 *     is not 8-byte aligned: GACQ_ERR_BAD_ARG, an unknown code GACQ_ERR_UNKNOWN_CODE; the message is gacq_last_error(NULL).
 *     gacq_scene_dev makes the same checks and reports an unknown PRN (GACQ_ERR_BAD_PRN) before it allocates or launches anything.
 *     Outputs are untouched after a refusal.  One launch on the ctx stream, no state kept; asynchronous.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_scene_emitter {
  int kind;                        /* 0 tone, 1 sawtooth chirp, 2 triangle chirp, 3 broadband noise */
  int pad;
  double amp;                      /* amplitude per component, LSB; kind 3: sigma per component */
  double f0_hz;                    /* frequency in the recording, Hz (chirps: at the start of a sweep); unused by kind 3 */
  double f1_hz;                    /* chirps: the frequency the ramp ends at */
  double phase;                    /* phase at j = 0, turns */
  long long sweep;                 /* chirps: P, samples per sweep */
  long long gate_period;           /* 0: always on */
  long long gate_on;               /* samples on per period */
  long long gate_first;            /* first sample of an on-interval */
} gacq_scene_emitter;

int gacq_scene_check(const gacq_sim_sat* sats, int K, const gacq_scene_emitter* emitters, int I, const double* gains, double fs, double sigma,
                     long long first_antenna, int M, long long j0, long long n, int out_complex64, void* const* d_out);
int gacq_scene_dev(gacq_ctx* ctx, const gacq_sim_sat* sats, int K, const gacq_scene_emitter* emitters, int I, const double* gains, double fs,
                   double sigma, unsigned long long seed, long long first_antenna, int M, long long j0, long long n, int out_complex64,
                   void* const* d_out);

/* ---------------------------------------------------------------------------------------------
 * Recording ingest (gacq_ingest.hip): packed, 8-bit, 16-bit and float32 recordings, I/Q or real IF, to the interleaved signed 8-bit
 * I/Q (or complex64) that every other entry point takes.  Output sample m is an exact function of (format, gain, absolute sample
 * index m) -- the same bytes however a caller cuts the recording into calls.
 * Values.  A container turns the bytes at d_in into values v[0], v[1], ...:
 *     GACQ_INGEST_S8 the int8; GACQ_INGEST_U8 byte - 128; GACQ_INGEST_S16 little-endian int16; GACQ_INGEST_F32 little-endian float32;
 *     GACQ_INGEST_PACKED: bits = 1, 2 or 4 per code, 8 / bits codes per byte; code i of a byte is (byte >> (8 - bits (i + 1))) & (2^bits - 1)
 *       with msb_first, (byte >> (bits i)) & (2^bits - 1) without; v = lut[code].
 * I/Q (real = 0): sample j is u(j) = v[2j] + i v[2j + 1].
 * Real IF (real != 0; S8, U8 and PACKED only, so |v| <= 128): x[n] = v[n], x[n] = 0 for n < 0; an fs/4 down-shift, a half-band low-pass
 * and decimation by two, all in integers (Gaussian integers, int32 per component):
 *     acc(m) = sum_{k = -21..21} g[k] x[2m - k] (-i)^(2m - k),        u(m) = acc(m) 2^-14,
 *     g[-k] = g[k], g[0] = 16384, g[even k != 0] = 0, g[1, 3, .., 21] = 10382, -3333, 1852, -1175, 774, -506, 320, -188, 97, -40, 9:
 *     rint(16384 h[k] / h[0]) of the 47-tap Hann-windowed sinc with its cutoff at fs/4 (gacq_firwin_hann(47, 0.5)); the taps sum to 32768.
 *   |acc| <= 128 * 53736 < 2^23, so u(m) is exact in fp32.  The output rate is fs/2 and a signal at IF f appears at f - fs/4.
 * conj != 0 negates the imaginary part of u (spectral inversion), in either mode.
 * Output: complex64 float32(u) * float32(gain) per component -- one fp32 multiply, nothing fused (out_complex64 != 0, d_out 8-byte
 * aligned) -- or interleaved int8 clip(rint(.), -127, 127) of exactly those values, ties to even, NaN to 0.
 * d_in holds input samples in_first .. in_first + in_count - 1 (a complex sample in I/Q mode, a real one in real mode) and starts on a
 * byte boundary: in_first times the bits per sample is a multiple of 8.  Output samples out_first .. out_first + n_out - 1 are written
 * to d_out; I/Q output m needs input m, real output m needs inputs 2m - 21 .. 2m + 21 (those below 0 are zero).  An input that is
 * needed and not present GACQ_ERR_SHORT_INPUT; an unknown container, bits outside {1, 2, 4}, real mode with S16 or F32, a gain that is
 * not finite and positive (as a double and as a float), a negative index or count or one above 2^48, an in_first off a byte boundary,
 * a misaligned complex64 d_out, a NULL pointer GACQ_ERR_BAD_ARG.  Everything is checked on the host before anything is launched.
 * n_out = 0 does nothing.  One launch on the ctx stream, no staging, no state; asynchronous.
 * ------------------------------------------------------------------------------------------- */
#define GACQ_INGEST_S8 0
#define GACQ_INGEST_U8 1
#define GACQ_INGEST_S16 2
#define GACQ_INGEST_F32 3
#define GACQ_INGEST_PACKED 4
typedef struct gacq_ingest_fmt {
  int container;                   /* GACQ_INGEST_* */
  int real;                        /* 0: I/Q pairs; otherwise real IF samples */
  int bits;                        /* PACKED: bits per code, 1, 2 or 4 */
  int msb_first;                   /* PACKED: the first code of a byte is in its top bits */
  int conj;                        /* negate the imaginary part */
  int pad[3];
  int8_t lut[16];                  /* PACKED: value of each code */
} gacq_ingest_fmt;

int gacq_ingest_dev(gacq_ctx* ctx, const gacq_ingest_fmt* fmt, const void* d_in, long long in_first, long long in_count,
                    long long out_first, long long n_out, double gain, int out_complex64, void* d_out);

/* ---------------------------------------------------------------------------------------------
 * Interference mitigation (gacq_mitigate.hip): a pulse blanker and a spectral excision filter on the canonical recording, interleaved
 * int8 I/Q (in_complex64 = 0) or complex64 in, int8 I/Q or complex64 out.  Every decision is a function of the absolute sample index, so
 * the output does not depend on how the recording is cut into calls.  Input x(j), j >= 0; x(j) = 0 for j < 0.
 * 1. Sanitise.  A sample with a non-finite component (complex64 input only) is replaced by 0 and counted as blanked, also with
 *    blanking off; it is no hit below.
 * 2. Blanking (blank_thr > 0).  p(j) = re^2 + im^2: int32 for int8 input; fp32 re*re + im*im, nothing fused, for complex64.
 *    hit(j) = p(j) > blank_thr^2, the square formed once on the host in the arithmetic of the comparison: floor(blank_thr^2) of the
 *    double for int8 input, float(blank_thr) * float(blank_thr) in fp32 for complex64.
 *    z(j) = 0 when hit(j + d) holds for some |d| <= hold (0..64), else x(j).  Without blanking z = the sanitised x.
 * 3. Excision (nfft != 0).  N = nfft a power of two in 64..4096, H = N / 2, w[n] = sin(pi (n + 0.5) / N) (w[n]^2 + w[n + H]^2 = 1).
 *    Frame f >= 0 covers inputs (f - 1) H .. (f + 1) H - 1:  X_f = FFT_N(w z),  P_f[k] = |X_f[k]|^2,  med_f = the (N/2)-th smallest of
 *    the N values P_f[k] (1-based: the lower median).  Bin k is hit when P_f[k] > ratio med_f (strict: an all-zero frame excises
 *    nothing); every hit bin and its `guard` (0..8) neighbours on either side, circular in k, are set to 0.  y_f = w IFFT_N(X_f).
 *    Output sample j of block q = j div H is y_q[j - (q - 1) H] + y_{q+1}[j - q H].  Without excision y = z.
 * 4. Output, as in ingest: complex64 float32(y) * float32(gain) per component, one multiply, nothing fused; or int8
 *    clip(rint(.), -127, 127) of exactly that value, ties to even, NaN to 0.
 * 5. Statistics.  d_stats (NULL, or three uint64 that the caller zeroed; added to with integer atomics): [0] blanked = the samples j of
 *    the output range whose z(j) was forced to 0 (sanitised or under a hit's hold); [1] frames = the frames f with
 *    out_first <= f H < out_first + n_out (the frames the call owns); [2] bins = the zeroed bins over the owned frames.  d_frame_bins
 *    (NULL, or one uint32 per owned frame, in frame order) receives each owned frame's zeroed-bin count.  The totals of any partition
 *    of the outputs into calls sum to those of one call.
 * d_in holds input samples in_first .. in_first + in_count - 1.  With excision, output block q needs inputs (q - 1) H - hold ..
 * (q + 2) H - 1 + hold; without, output j needs j - hold .. j + hold; inputs below 0 are zero.  A needed input that is not present
 * GACQ_ERR_SHORT_INPUT: a recording ends at the last output whose support is present.  Both stages off, nfft not a power of two in
 * 64..4096, a ratio that is not finite or <= 1, blank_thr negative or not finite, hold outside 0..64, guard outside 0..8, a gain that is
 * not finite and positive (as a double and as a float), an index or count below 0 or above 2^48, a complex64 buffer off 8 bytes, a NULL
 * cfg / d_in / d_out GACQ_ERR_BAD_ARG.  Everything is checked on the host before anything is launched (gacq_mitigate_check makes the
 * same checks and needs no context); a refused call leaves d_out and d_stats untouched.  n_out = 0 does nothing.  One launch on the
 * ctx stream, asynchronous.  gacq_mitigate_tile: the output blocks one workgroup of the excision kernel owns (for tests), or
 * GACQ_ERR_BAD_ARG for a length the kernel does not serve.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_mitigate_cfg {
  double blank_thr;                /* amplitude threshold of the blanker; 0: blanking off */
  double ratio;                    /* excision threshold over the frame's median power, > 1 */
  int hold;                        /* samples blanked on either side of a hit, 0..64 */
  int nfft;                        /* frame length, a power of two in 64..4096; 0: excision off */
  int guard;                       /* bins zeroed on either side of a hit bin, 0..8 */
  int pad;
} gacq_mitigate_cfg;

int gacq_mitigate_tile(int nfft);
int gacq_mitigate_check(const gacq_mitigate_cfg* cfg, const void* d_in, int in_complex64, long long in_first, long long in_count,
                        long long out_first, long long n_out, double gain, int out_complex64, const void* d_out);
int gacq_mitigate_dev(gacq_ctx* ctx, const gacq_mitigate_cfg* cfg, const void* d_in, int in_complex64, long long in_first, long long in_count,
                      long long out_first, long long n_out, double gain, int out_complex64, void* d_out, void* d_stats, void* d_frame_bins);

/* ---------------------------------------------------------------------------------------------
 * Digital down-converter (gacq_ddc.hip): a band out of a wide recording.  A mixer, an integer FIR low-pass and integer decimation;
 * interleaved int8 I/Q in, int8 I/Q or complex64 out.  Output sample m is an exact function of (configuration, gain, absolute sample
 * index), so the output does not depend on how the recording is cut into calls.  All arithmetic is integer up to the last multiply.
 * NCO.  dphase = dP = rint(f_shift / fs * 2^64) mod 2^64 (the caller forms it; gnss_dsp_tools_amd/ddc.py does so exactly).  Phase word
 *     P(n) = (n dP) mod 2^64 of absolute input sample n; table index t(n) = P(n) >> 52; table W[t] = (rint(16384 cos(2 pi t / 4096)),
 *     rint(16384 sin(2 pi t / 4096))), t < 4096, int16, formed on the host in double (gacq_ddc_table writes the 8192 values, cos first).
 *     The shift applied is f_act = dP_signed / 2^64 * fs (dP_signed: dP as a signed 64-bit number); a signal at carrier offset c
 *     appears at c - f_act.
 * Mixed sample.  x(n) the input as a Gaussian integer, x(n) = 0 for n < 0;  p(n) = x(n) conj(W[t(n)]);  z(n) = (p(n) + 64) >> 7 per
 *     component, arithmetic shift.  |z| <= 23171 per component: an int16 pair.
 * Filter and decimation.  Taps g[-H .. H], integers handed over as int32 words (the one-tap filter of a pure shift is g = 32768, one
 *     more than an int16 holds), T = 2 H + 1 odd in 1..513, sum |g| <= 65536, not required to be symmetric; taps[i] is g[i - H].
 *     decim = D in 1..64.   acc(m) = sum_{k = -H..H} g[k] z(m D - k)    per component, int32: |acc| < 23171 * 65536 < 2^31,
 *     exact in any order.  Output m is centred on input m D: no group delay.  The output rate is fs / D.
 * Output.  v = float32(acc) (round to nearest even); complex64 v * s with s = float32(gain) * 2^-22, one fp32 multiply per component,
 *     nothing fused (taps that sum to 32768 have unity gain at gain 1); or int8 clip(rint(.), -127, 127) of exactly those values, ties to
 *     even.
 * d_in holds input samples in_first .. in_first + in_count - 1; output samples out_first .. out_first + n_out - 1 are written to d_out.
 * Output m needs inputs m D - H .. m D + H, those below 0 being zero; one that is needed and not present GACQ_ERR_SHORT_INPUT: a
 * recording of N samples ends at output (N - 1 - H) div D.  D or T out of range, T even, sum |g| > 65536, a gain that is not finite and
 * positive (as a double and as a float), an index or count below 0 or above 2^48, a NULL pointer, a complex64 d_out off 8 bytes
 * GACQ_ERR_BAD_ARG.  Everything is checked on the host before the launch; a refused call leaves d_out untouched; n_out = 0 does nothing.
 * gacq_ddc_open uploads the table and the taps once (it may wait for the device); gacq_ddc_run_dev is one asynchronous launch on the
 * ctx stream, without synchronisation or state; the handle is closed before its context is destroyed.  gacq_ddc_check makes every
 * check that needs no pointer to device memory, without a device.  gacq_ddc_tile: the outputs one workgroup owns (for tests), or
 * GACQ_ERR_BAD_ARG for a D outside 1..64.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_ddc_cfg {
  unsigned long long dphase;       /* dP: the NCO's phase increment per input sample, in units of 2^-64 cycles */
  int decim;                       /* D, 1..64 */
  int pad;
} gacq_ddc_cfg;
typedef struct gacq_ddc gacq_ddc;

int gacq_ddc_tile(int decim);
int gacq_ddc_table(int16_t* table);
int gacq_ddc_check(const gacq_ddc_cfg* cfg, const int32_t* taps, int T, long long in_first, long long in_count, long long out_first,
                   long long n_out, double gain, int out_complex64);
int gacq_ddc_open(gacq_ctx* ctx, const gacq_ddc_cfg* cfg, const int32_t* taps, int T, gacq_ddc** out);
int gacq_ddc_run_dev(gacq_ddc* h, const void* d_in, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                     int out_complex64, void* d_out);
void gacq_ddc_close(gacq_ddc* h);

/* ---------------------------------------------------------------------------------------------
 * Level control and requantiser (gacq_requant.hip): the inverse of ingest.  Interleaved integer I/Q in, any ingest container out,
 * under a gain that follows the block power of the recording.  Every decision is an integer function of the absolute block index, so
 * the bytes do not depend on how the recording is cut into calls.
 * Input.  x(j), j >= 0: interleaved I/Q, in_bits = 8 (int8) or 16 (little-endian int16, d_in 2-byte aligned).
 * 1. Block power.  block = Lb, a multiple of 16 in 16..65536; block b covers samples b Lb .. (b + 1) Lb - 1.
 *    P(b) = sum re^2 + im^2 over the block, an exact unsigned 64-bit integer (P(b) <= Lb 2^31).
 * 2. Level.  window = W in 1..64.  S(b) = P(b - W) + .. + P(b - 1) for b >= W; S(b) = P(0) + .. + P(W - 1) for b < W (the warm-up).
 *    S(b) <= 2^53.  Causal and not recursive: a function of b alone.
 * 3. Gain.  ngains = K in 1..256; gains G[0 .. K-1], float32, each finite and positive; thresholds T[0] <= T[1] <= .. <= T[K-2],
 *    unsigned 64-bit (host arrays; thresholds may be NULL when K = 1).  k(b) = the number of i with S(b) > T[i] (strict), g(b) = G[k(b)].
 *    The library forms no table: it checks order and finiteness only.  K = 1 is a fixed gain.
 * 4. Value.  v = float32(component) * g(j div Lb): one fp32 multiply per component, nothing fused.
 * 5. Output container (the GACQ_INGEST_* numbers):
 *     S8      clip(rint(v), -127, 127), ties to even: the canonical int8;     U8   that value plus 128;
 *     S16     clip(rint(v), -32767, 32767), little-endian (d_out 2-byte aligned);     F32  v itself, complex64 (d_out 8-byte aligned);
 *     PACKED  bits in {1, 2, 4}, n = 2^bits: level index q = clip(floor(v * 0.5f) + n/2, 0, n - 1), which stands for the odd integer
 *             2q - (n - 1) (v in [0, 2) gives +1); code enc[q], enc a permutation of 0 .. n-1; codes in the order I0, Q0, I1, Q1, ..,
 *             8 / bits to a byte, code i of a byte at bit 8 - bits (i + 1) with msb_first, at bits i without: ingest's positions.
 *             out_first and n_out are multiples of the samples per byte, 4 / bits.
 * 6. Statistics.  d_stats (NULL, or two uint64 that the caller zeroed, 8-byte aligned; added to with vector integer atomics):
 *    [0] the components of the output range that the clip changed (PACKED: q clipped; F32: none); [1] the owned blocks, those with
 *    out_first <= b Lb < out_first + n_out.  d_gain_index (NULL, or one uint8 k(b) per owned block, in block order).  The totals of any
 *    partition of the outputs into calls sum to those of one call.
 * d_in holds input samples in_first .. in_first + in_count - 1; output samples out_first .. out_first + n_out - 1 are written to d_out.
 * Output j in block b needs input j and inputs max(b - W, 0) Lb .. max(b, W) Lb - 1; one that is needed and not present
 * GACQ_ERR_SHORT_INPUT: a recording shorter than W blocks gives no output, and the last partial block is produced.  A value outside
 * the ranges above, an unknown container, enc not a permutation, T not ascending, a gain that is not finite and positive, an index or
 * count below 0 or above 2^48, a misaligned int16 or complex64 buffer or d_stats, a NULL pointer GACQ_ERR_BAD_ARG.  Everything is
 * checked on the host before anything is launched; a refused call leaves d_out and d_stats untouched; n_out = 0 does nothing.
 * gacq_requant_check makes every check that needs no device pointer, without a context.  gacq_requant_open uploads the tables once
 * and allocates the handle's workspace (it may wait for the device); gacq_requant_run_dev is two launches (block powers, then the
 * outputs) per 2^16 blocks on the ctx stream, asynchronous, without state between calls: calls on one handle are ordered by that
 * stream.  The handle is closed before its context is destroyed.  gacq_requant_tile: the outputs one workgroup owns (for tests), or
 * GACQ_ERR_BAD_ARG.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_requant_cfg {
  int in_bits;                     /* 8: int8 input; 16: little-endian int16 */
  int container;                   /* output: GACQ_INGEST_* */
  int bits;                        /* PACKED: bits per code, 1, 2 or 4 */
  int msb_first;                   /* PACKED: the first code of a byte is in its top bits */
  int block;                       /* Lb: samples per power block, a multiple of 16 in 16..65536 */
  int window;                      /* W: blocks the level sums over, 1..64 */
  int ngains;                      /* K: entries of the gain table, 1..256 */
  int pad;
  uint8_t enc[16];                 /* PACKED: code of each level index, a permutation of 0 .. 2^bits - 1 */
} gacq_requant_cfg;
typedef struct gacq_requant gacq_requant;

int gacq_requant_tile(const gacq_requant_cfg* cfg);
int gacq_requant_check(const gacq_requant_cfg* cfg, const float* gains, const uint64_t* thresholds, long long in_first, long long in_count,
                       long long out_first, long long n_out);
int gacq_requant_open(gacq_ctx* ctx, const gacq_requant_cfg* cfg, const float* gains, const uint64_t* thresholds, gacq_requant** out);
int gacq_requant_run_dev(gacq_requant* h, const void* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                         void* d_out, void* d_stats, void* d_gain_index);
void gacq_requant_close(gacq_requant* h);

/* ---------------------------------------------------------------------------------------------
 * Cancellation of tracked signals (gacq_cancel.hip): rebuild known spread-spectrum signals from per-segment parameters and take them
 * out of a recording, interleaved int8 I/Q (in_complex64 = 0) or complex64 in, int8 I/Q or complex64 out.  Output sample j is a
 * function of (segments, amplitudes, x(j), j) only: the same bytes however a caller cuts the recording into calls and wherever d_in and
 * d_out lie.
 * A satellite is (code, prn, kind) as in gacq_sim_sat, followed by the number of its segments; segs holds the segments of satellite 0,
 * then those of satellite 1, and so on.  A segment says how its satellite's signal runs over samples s0 .. s0 + n - 1 of the recording
 * (absolute indices).  The doubles become fixed point once on the host, by the rules of gacq_simulate_dev:
 *     F = floor(frac(carrier_hz / fs) 2^64), p0 = floor(frac(carrier_phase) 2^64)   (carrier_phase: turns at s0)
 *     Cf = floor((code_rate_hz / fs) 2^64),  c0 = floor(code_phase 2^64)            (code_phase: chips at s0, in [0, L))
 * and for i = j - s0
 *     theta(j) = (p0 + i F) mod 2^64,   pos(j) = c0 + i Cf   (exact integer: chip (pos >> 64) mod L, subchip fraction pos mod 2^64)
 *     r(j) = w(pos(j)) exp(2 pi i theta(j) / 2^64)           (w: simulate's chip weight of `kind` at unit amplitude, no symbols)
 * The segments of one satellite ascend in s0 and do not overlap; nothing of a satellite is subtracted in a gap between its segments.
 * Estimate (estimate != 0).  For every segment that touches the output range:
 *     C = sum_j x(j) conj(r(j)),   E = sum_j w(pos(j))^2,   A = C / E (0 when E = 0)
 *   with fp32 products (w cos, w sin; re = xr rr + xi ri, im = xi rr - xr ri; w w; each product and sum rounded on its own) and fp64 sums
 *   in an order that depends on i alone: the bits of A are a function of the segment and its own samples, not of the call, the other
 *   segments or the addresses.  Every amplitude is estimated on the input, never on a partly cancelled signal (parallel cancellation).
 *   Without the flag A = (amp_re, amp_im).
 * Subtract.  v(j) = x(j) - sum_k float32(A_k) r_k(j) in fp32, one satellite after the other in ascending k, over the satellites that
 *   have a segment covering j.
 * d_out (device): complex64 v (out_complex64 != 0, 8-byte aligned), or interleaved int8 clip(rint(v), -127, 127) with ties to even, of
 * the very values the complex64 form holds.  The int8 rule is applied to every sample, covered or not: an input of -128 comes out as
 * -127.  d_in holds input samples in_first .. in_first + in_count - 1; outputs out_first .. out_first + n_out - 1 are written.
 * amps_out (host, NULL or one complex128 per segment): A of every segment that touches the output range; the other entries are left as
 * they are.  clipped (host, NULL or one count): the components of an int8 output that are +127 or -127 (0 for complex64 output).
 * Limits: K in 1..32, at most 2^20 segments, n in 1..2^24, codes of at most 10240 chips, indices and counts at most 2^48.
 * Checked on the host before anything is allocated or launched (gacq_cancel_check makes the same checks and needs no context): a value
 * that is not finite, fs <= 0, code_rate_hz <= 0 or code_rate_hz / fs >= 16, code_phase outside [0, L), kind outside 0..5, K, a segment
 * count, n, an index or a count out of range, overlapping or unsorted segments, a complex64 buffer off 8 bytes, a NULL pointer
 * GACQ_ERR_BAD_ARG; an unknown code or PRN GACQ_ERR_UNKNOWN_CODE / GACQ_ERR_BAD_PRN; a code longer than 10240 chips
 * GACQ_ERR_UNSUPPORTED; an output sample whose input is not present, or with estimate a segment that touches the output range and does
 * not lie wholly inside the input, GACQ_ERR_SHORT_INPUT.  A refused call leaves d_out untouched; n_out = 0 does nothing.  Up to two
 * launches on the ctx stream; the call returns when the results are there.
 * Prompts across an antenna array (gacq_aprompt.hip, gacq_aprompt_dev): the estimate alone, of M recordings on one sample clock against
 * the same satellites and segments.  antennas = M in 1..8; d_in is a host array of M device pointers, row p holding input samples
 * in_first .. in_first + in_count - 1 of antenna p, interleaved int8 I/Q at any byte address or complex64 8-byte aligned (the
 * convention of gacq_null_run_dev; two antennas may share a pointer).  amp_re and amp_im are not looked at.  For every segment that
 * lies wholly inside the input range and every antenna p
 *     C_p = sum_j x_p(j) conj(r(j)),   E = sum_j w(pos(j))^2,   A_p = C_p / E (0 when E = 0)
 *   with the operations of the estimate above: the same fixed-point phase and code position, the same fp32 products each rounded on
 *   its own, the same order of the fp64 sums (sample i of the segment to lane i mod 256, a lane adds in ascending i, lanes by DPP row
 *   sums and a fixed LDS tree).  A_p is bit for bit the A that gacq_cancel_dev (estimate) returns for that segment on antenna p's
 *   recording alone: the bits depend on the segment and its own samples, not on M, the other antennas, the call, the other segments
 *   or the addresses.  The replica of a sample is built once for all M antennas.
 * prompts_out (host): complex fp64 [segment][antenna][2]; energy_out (host, or NULL): E, fp64 [segment].  A segment that is not wholly
 * inside the input is left untouched in both (callers prefill, e.g. with NaN): no error, and nothing outside the rows is read.
 * Limits and checks are those above, and antennas outside 1..8, a NULL row, a complex64 row off 8 bytes, a NULL prompts_out
 * GACQ_ERR_BAD_ARG (gacq_aprompt_check makes the checks that need no context).  A refused call launches nothing and writes nothing.
 * One launch on the ctx stream; the call returns when the results are there.
 * The replica, the device tables and the host preparation of both entry points are csrc/gacq_cancelcore.h.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_cancel_sat {
  const char* code;                /* code module, e.g. "gps.ca" */
  int prn;                         /* PRN (GLONASS: 0) */
  int kind;                        /* chip weight, 0 plain .. 5 RZ [0,1] */
  int nseg;                        /* segments of this satellite in segs, >= 0 */
  int pad;
} gacq_cancel_sat;
typedef struct gacq_cancel_seg {
  long long s0;                    /* first sample (absolute index) */
  long long n;                     /* samples, 1..2^24 */
  double carrier_hz;               /* carrier frequency in the recording, Hz */
  double carrier_phase;            /* carrier phase at s0, turns */
  double code_rate_hz;             /* chips per second */
  double code_phase;               /* code phase at s0, chips, in [0, L) */
  double amp_re, amp_im;           /* complex amplitude (used when estimate = 0) */
} gacq_cancel_seg;

int gacq_cancel_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, int estimate, const void* d_in, int in_complex64,
                      long long in_first, long long in_count, long long out_first, long long n_out, int out_complex64, const void* d_out);
int gacq_cancel_dev(gacq_ctx* ctx, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, int estimate, const void* d_in,
                    int in_complex64, long long in_first, long long in_count, long long out_first, long long n_out, int out_complex64, void* d_out,
                    double* amps_out, unsigned long long* clipped);
int gacq_aprompt_check(const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, const void* const* d_in, int antennas,
                       int in_complex64, long long in_first, long long in_count);
int gacq_aprompt_dev(gacq_ctx* ctx, const gacq_cancel_sat* sats, int K, const gacq_cancel_seg* segs, double fs, const void* const* d_in,
                     int antennas, int in_complex64, long long in_first, long long in_count, double* prompts_out, double* energy_out);

/* ---------------------------------------------------------------------------------------------
 * Spatial nulling with an antenna array (gacq_null.hip): M recordings on one sample clock in, one recording out, under weights that
 * minimise the output power of every block subject to one linear constraint.  Every decision is a function of the absolute block index,
 * so the bytes do not depend on how the recording is cut into calls.
 * Input.  antennas = M in 2..8.  x_p(j), p < M, j >= 0: interleaved int8 I/Q as stored (-128 is a legal value).  d_in is a host array
 *    of M device pointers, each at any byte address; two antennas may share a pointer.
 * 1. Block covariance.  block = Lb, a multiple of 64 in 64..32768; block b covers samples b Lb .. (b + 1) Lb - 1.
 *    C_b[p][q] = sum x_p(j) conj(x_q(j)) over the block, a Gaussian integer.  With the real rows r_2p = I_p, r_2p+1 = Q_p and
 *    G[u][v] = sum r_u r_v (|G| <= 2^29):  Re C[p][q] = G[2p][2q] + G[2p+1][2q+1],  Im C[p][q] = G[2p+1][2q] - G[2p][2q+1]
 *    (Im C[p][p] is exactly 0; every component fits int32).
 * 2. Window.  window = W in 1..64.  R_b = C_(b-W) + .. + C_(b-1) for b >= W; R_b = C_0 + .. + C_(W-1) for b < W (the warm-up).  int64,
 *    exact, a function of b alone.
 * 3. Loading.  t = sum_p Re R_b[p][p];  d = (t >> load_shift) + 1, load_shift in 0..40 (10 where a caller has no reason for another);
 *    A = R_b + d I, every entry converted to fp64 (exact: below 2^53).  d >= 1 keeps A positive definite for all-zero input and for
 *    antennas that share a buffer.
 * 4. Weights.  c: M complex doubles (c[2p], c[2p+1] = re, im), all finite, not all zero; (1, 0, .., 0) is power inversion with antenna
 *    0 as the reference, any other c an MVDR steering vector.  Complex fp64, every real product and every real sum rounded on its own,
 *    nothing fused; (a + ib)(c + id) = (ac - bd) + i(ad + bc); z / real = (re / real) + i(im / real), two divisions.
 *      b = c.   for k = 0 .. M-1:  piv_k = Re A[k][k];  for r = k+1 .. M-1:  m = A[r][k] / piv_k;
 *                                     for q = k+1 .. M-1:  A[r][q] = A[r][q] - m A[k][q];      b[r] = b[r] - m b[k]
 *      for k = M-1 .. 0:  s = b[k];  for q = k+1 .. M-1 (ascending):  s = s - A[k][q] u[q];      u[k] = s / piv_k
 *      den = t_0 + t_1 + .. + t_(M-1) (left to right),  t_p = Re c_p Re u_p + Im c_p Im u_p;      w_p = u_p / den
 *    (Gaussian elimination without pivoting; A - m A[k] is a componentwise subtraction of the product.)  c^H w = 1: with the default c
 *    the reference antenna passes with gain 1.
 * 5. Quantised weights.  Per component wq = clamp(rint(w 2^14), -131071, 131071), ties to even, 0 when w 2^14 is not finite; int32 pairs.
 * 6. Apply.  y(j) = sum_p conj(wq_p(j div Lb)) x_p(j):  re = sum wr xr + wi xi,  im = sum wr xi - wi xr, in int32 (|.| < 2^28, exact in
 *    any order).
 * 7. Output.  v = float32(component) (round to nearest even); complex64 v * s with s = float32(gain) * 2^-14 (formed in fp32), one fp32
 *    multiply per component, nothing fused; or int8 clip(rint(.), -127, 127) of exactly those values, ties to even.
 * 8. Side outputs, each NULL or device memory.  d_stats: two uint64 that the caller zeroed, 8-byte aligned, added to with vector integer
 *    atomics: [0] the components of an int8 output that the clip changed (0 for complex64), [1] the owned blocks, those with
 *    out_first <= b Lb < out_first + n_out; the totals of any partition of the outputs into calls sum to those of one call.
 *    d_weights: wq of every owned block in block order, int32 [block][M][2].  d_cov: R_b of every owned block, int64 [block][M][M][2].
 * d_in[p] holds input samples in_first .. in_first + in_count - 1 of antenna p; output samples out_first .. out_first + n_out - 1 are
 * written to d_out.  Output j in block b needs x_p(j) of every antenna and inputs max(b - W, 0) Lb .. max(b, W) Lb - 1; one that is
 * needed and not present GACQ_ERR_SHORT_INPUT: a recording shorter than W blocks gives no output, and the last partial block is
 * produced.  A value outside the ranges above, a c that is not finite or all zero, a gain that is not finite and positive (as a double
 * and as a float), an index or count below 0 or above 2^48, a complex64 d_out or a d_stats off 8 bytes, a d_weights off 4 or a d_cov
 * off 8 bytes, a NULL pointer (d_in, one of its entries, d_out) GACQ_ERR_BAD_ARG.  Everything is checked on the host before anything is
 * launched; a refused call leaves every output untouched; n_out = 0 does nothing.
 * gacq_null_check makes every check that needs no device pointer, without a context.  gacq_null_open allocates the handle's workspace
 * (it may wait for the device); gacq_null_run_dev is three launches (block covariances, weights, outputs) per 2^14 blocks on the ctx
 * stream, asynchronous, without state between calls and without host synchronisation: calls on one handle are ordered by that stream.
 * The handle is closed before its context is destroyed.  gacq_null_tile: the output samples one workgroup owns (for tests; tiles begin
 * at absolute sample indices that are multiples of it, a lane's run of 8 samples at multiples of 8), or GACQ_ERR_BAD_ARG.
 * The host path (these checks, the handle, the chunk loop) is csrc/gacq_arrayhost.h, which gacq_stap below shares.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_null_cfg {
  int antennas;                    /* M, 2..8 */
  int block;                       /* Lb: samples per covariance block, a multiple of 64 in 64..32768 */
  int window;                      /* W: blocks the covariance sums over, 1..64 */
  int load_shift;                  /* diagonal loading d = (trace >> load_shift) + 1, 0..40 */
  double c[16];                    /* the constraint: re, im of c_0 .. c_(M-1); the rest is ignored */
} gacq_null_cfg;
typedef struct gacq_null gacq_null;

int gacq_null_tile(const gacq_null_cfg* cfg);
int gacq_null_check(const gacq_null_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                    int out_complex64);
int gacq_null_open(gacq_ctx* ctx, const gacq_null_cfg* cfg, gacq_null** out);
int gacq_null_run_dev(gacq_null* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                      double gain, int out_complex64, void* d_out, void* d_stats, void* d_weights, void* d_cov);
void gacq_null_close(gacq_null* h);

/* ---------------------------------------------------------------------------------------------
 * Space-time adaptive nulling (gacq_stap.hip): gacq_null with T taps on every antenna.  The weight vector has N = M T entries, so
 * narrowband interferers are separated in frequency as well as in direction; with M = 1 it is an adaptive FIR notch.  Every decision is
 * a function of the absolute block index, so the bytes do not depend on how the recording is cut into calls.
 * Input.  antennas = M in 1..8; taps = T, odd, in 1..15; N = M T <= 56 (the int32 apply stays below 2^31: 112 * 131071 * 128 = 1.879e9).
 *    t_c = (T - 1) / 2.  x_p(j), p < M: interleaved int8 I/Q as stored (-128 is a legal value); x_p(i) = 0 for i < 0.  d_in is a host
 *    array of M device pointers, each at any byte address; two antennas may share a pointer.
 * Stacked sample.  Element e = p T + t (antenna-major), t < T:  z_e(j) = x_p(j + t_c - t).  The reference element is e_ref = t_c,
 *    z_(t_c)(j) = x_0(j): the output keeps the recording's sample index.
 * 1. Block covariance.  block = Lb, window = W, load_shift as in gacq_null_cfg.  C_b[e][f] = sum z_e(j) conj(z_f(j)) over the samples j
 *    of block b: the exact sum of the stacked vectors (no Toeplitz approximation; the taps reach t_c samples into the neighbouring
 *    blocks), formed through the Gram matrix of the 2N real rows as in gacq_null (|G| <= 2^29, every component fits int32).
 * 2.-5. Window, loading, weights, quantised weights.  Steps 2 to 5 of gacq_null with M replaced by N: R_b in int64, d = (trace R_b >>
 *    load_shift) + 1, A u = c by the same elimination without pivoting and back substitution in the same written-out order, every real
 *    product and sum rounded on its own, den summed left to right over all N entries, wq = clamp(rint(w 2^14), +-131071).  The
 *    elimination updates the whole trailing submatrix (q and r from k + 1 to N - 1): in fp64 the trailing matrix is not exactly
 *    Hermitian, so the lower triangle is computed, not mirrored.  The constraint c of the N-vector: the M complex entries of the
 *    configuration on the centre taps, c_(p T + t_c) = (c[2p], c[2p+1]), every other entry zero; the default (1, 0, ..) is power
 *    inversion with x_0(j) at gain exactly 1.
 * 6. Apply.  y(j) = sum_e conj(wq_e(j div Lb)) z_e(j) in int32, with the weights of j's own block; the taps reach across block edges
 *    into the neighbours' samples.
 * 7., 8. Output and side outputs as gacq_null: complex64 or int8 clip(rint(.), -127, 127); d_stats; d_weights int32 [owned block][N][2];
 *    d_cov int64 [owned block][N][N][2].
 * Support.  Output j in block b needs x_p(max(j - t_c, 0) .. j + t_c) and blocks max(b - W, 0) .. max(b, W) - 1 with t_c samples either
 *    side (samples below 0 do not exist and are not needed): outputs out_first .. out_first + n_out - 1 need inputs
 *    max(max(out_first div Lb - W, 0) Lb - t_c, 0) .. max(out_first + n_out, W Lb) - 1 + t_c.  A recording of n samples supports outputs
 *    0 .. n - 1 - t_c, and none until n >= W Lb + t_c.  One that is needed and not present GACQ_ERR_SHORT_INPUT.  Nothing outside
 *    in_first .. in_first + in_count - 1 of any antenna is read.
 * The checks, their order, "a refused call leaves every output untouched", n_out = 0, the 2^48 limits and the alignment rules of the
 * side outputs are those of gacq_null; taps even or outside 1..15 and M T > 56 GACQ_ERR_BAD_ARG, checked after the antennas and
 * before the block.  With M >= 2 and T = 1 every byte, weight, window sum and count equals gacq_null_run_dev's.
 * gacq_stap_check makes every check that needs no device pointer, without a context.  gacq_stap_open allocates the handle's workspace,
 * gacq_stap_workspace bytes: ((K + W) N^2 + K N) * 8 with K = min(2^14, (2^26 - 8 W N^2) div (8 N^2 + 8 N)) blocks per triple of
 * launches, at most 64 MiB.  gacq_stap_run_dev is three launches (block covariances, weights, outputs) per K blocks on the ctx stream,
 * asynchronous, without state between calls and without host synchronisation.  The handle is closed before its context is destroyed.
 * gacq_stap_tile: the output samples one workgroup owns (tiles begin at absolute sample indices that are multiples of it, a lane's run
 * of 8 samples at multiples of 8), or GACQ_ERR_BAD_ARG.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_stap_cfg {
  int antennas;                    /* M, 1..8 */
  int taps;                        /* T, odd, 1..15; M T <= 56 */
  int block;                       /* Lb: samples per covariance block, a multiple of 64 in 64..32768 */
  int window;                      /* W: blocks the covariance sums over, 1..64 */
  int load_shift;                  /* diagonal loading d = (trace >> load_shift) + 1, 0..40 */
  double c[16];                    /* the constraint: re, im of c_0 .. c_(M-1), on the centre taps; the rest is ignored */
} gacq_stap_cfg;
typedef struct gacq_stap gacq_stap;

int gacq_stap_tile(const gacq_stap_cfg* cfg);
long long gacq_stap_workspace(const gacq_stap_cfg* cfg);
int gacq_stap_check(const gacq_stap_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out, double gain,
                    int out_complex64);
int gacq_stap_open(gacq_ctx* ctx, const gacq_stap_cfg* cfg, gacq_stap** out);
int gacq_stap_run_dev(gacq_stap* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                      double gain, int out_complex64, void* d_out, void* d_stats, void* d_weights, void* d_cov);
void gacq_stap_close(gacq_stap* h);

/* ---------------------------------------------------------------------------------------------
 * Per-satellite beams (gacq_beams.hip): gacq_null with K constraints at once.  M recordings in, K recordings out; output k is formed
 * under the block-wise minimum-power weights of constraint c_k (an MVDR beam toward the steering vector c_k, as arrayprompt measures
 * it).  The block covariance, the window and the loading do not depend on the constraint and are formed once for all K.
 * Input.  antennas = M in 2..8 and d_in as gacq_null; beams = K in 1..16; c[k] = (re, im) of the M entries of c_k, every c_k finite
 *    and not all zero; entries past M and rows past K are ignored.
 * 1.-3. Block covariance, window, loading.  Steps 1 to 3 of gacq_null, unchanged: C_b, R_b, A = R_b + d I.
 * 4.-7. For every beam k < K: steps 4 to 7 of gacq_null with c = c_k and gain = gain[k]: the weights, the quantised weights, the
 *    apply and the output d_out[k].
 * Contract.  Every byte of output k, its quantised weights and its clip count are bit for bit what gacq_null_run_dev writes for the
 *    same inputs and call range under constraint c_k and gain gain[k], whatever K, the other beams, their order and the output
 *    addresses are: the elimination of A never reads the right-hand side, and every operation on b in step 4 depends only on A's
 *    multipliers m = A[r][k] / piv_k, its pivots and b itself, so the forward pass on b_k after the elimination, with m formed again
 *    by the same division, gives the bits of the fused loop.
 * 8. Side outputs, each NULL or device memory.  d_stats: K + 1 uint64 that the caller zeroed, 8-byte aligned: [k] the components of
 *    int8 output k that the clip changed, [K] the owned blocks.  d_weights: int32 [owned block][K][M][2].  d_cov: gacq_null's, int64
 *    [owned block][M][M][2], independent of the beams.
 * gain is a host array of K doubles and d_out a host array of K device pointers, each at any byte address (complex64: on 8 bytes).
 * Outputs that overlap each other or an input are the caller's business: nothing is checked and the bytes of the overlap are
 * undefined.  The support rule, the limits and the alignment rules are those of gacq_null.  GACQ_ERR_BAD_ARG for everything
 * gacq_null refuses and for beams outside 1..16 (checked after the antennas), a c_k that is not finite or all zero (the message
 * names k), a gain[k] that is not finite and positive, a NULL gain, d_out or entry of d_out, a complex64 d_out[k] off 8 bytes.
 * Everything is checked on the host before anything is launched; a refused call leaves every output untouched; n_out = 0 does
 * nothing.  gacq_beams_check, gacq_beams_open (which also puts the constraints on the device), gacq_beams_close and gacq_beams_tile
 * are what their gacq_null counterparts are; gacq_beams_run_dev is three launches (block covariances -- gacq_null's own kernel --,
 * the weights of all beams, all outputs) per 2^14 blocks on the ctx stream.  The host path is csrc/gacq_arrayhost.h.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_beams_cfg {
  int antennas;                    /* M, 2..8 */
  int beams;                       /* K, 1..16 */
  int block;                       /* Lb: samples per covariance block, a multiple of 64 in 64..32768 */
  int window;                      /* W: blocks the covariance sums over, 1..64 */
  int load_shift;                  /* diagonal loading d = (trace >> load_shift) + 1, 0..40 */
  double c[16][16];                /* row k: re, im of the M entries of c_k; the rest is ignored */
} gacq_beams_cfg;
typedef struct gacq_beams gacq_beams;

int gacq_beams_tile(const gacq_beams_cfg* cfg);
int gacq_beams_check(const gacq_beams_cfg* cfg, long long in_first, long long in_count, long long out_first, long long n_out,
                     const double* gain, int out_complex64);
int gacq_beams_open(gacq_ctx* ctx, const gacq_beams_cfg* cfg, gacq_beams** out);
int gacq_beams_run_dev(gacq_beams* h, const void* const* d_in, long long in_first, long long in_count, long long out_first, long long n_out,
                       const double* gain, int out_complex64, void* const* d_out, void* d_stats, void* d_weights, void* d_cov);
void gacq_beams_close(gacq_beams* h);

/* ---------------------------------------------------------------------------------------------
 * Bearings of interferers (gacq_bearing.hip): the minimum-variance (Capon) spatial spectrum of every block's window covariance over a
 * grid of directions, and the K strongest peaks that lie apart.  Every result is a function of (configuration, tables, covariance
 * matrix) alone, so with gacq_null_run_dev's d_cov it is a function of the absolute block index.
 * Input.  antennas = M in 2..8, load_shift in 0..40, cells = G in 1..32768, peaks = K in 1..4, cos_sep a finite double in -1..1.  Two
 *    host tables, read by gacq_bearing_open (all trigonometry stays with the caller): a[g][p], the steering vector of cell g, complex
 *    fp64 [G][M][2]; u[g], its direction, fp64 [G][3]; every entry finite.  R: int64 [..][M][M][2], both triangles, the layout of
 *    gacq_null_run_dev's d_cov.  Evaluated block i < n takes row i stride of d_cov, stride >= 1.
 * 1. Loading.  Step 3 of gacq_null: t = sum_p Re R[p][p];  d = (t >> load_shift) + 1;  A = R + d I, every entry converted to fp64.
 * 2. Elimination.  For every cell g the elimination of gacq_null step 4 with b = a_g, in that order, every real product and sum
 *    rounded on its own, nothing fused, the complex product and the division by the real pivot as written there:
 *      for k = 0 .. M-1:  piv_k = Re A[k][k];  for r = k+1 .. M-1:  m = A[r][k] / piv_k;
 *                            for q = k+1 .. M-1:  A[r][q] = A[r][q] - m A[k][q];      b[r] = b[r] - m b[k]
 *    No back substitution.  (The matrix part does not depend on g.)
 * 3. Quadratic form.  q_g = t_0 + t_1 + .. + t_(M-1), left to right, t_k = ((Re b_k)^2 + (Im b_k)^2) / piv_k: two products, one sum,
 *    one division.  This is a_g^H A^-1 a_g; the Capon power 1 / q_g is left to the caller.
 * 4. Eligibility.  A cell is eligible when q_g is finite and > 0.  floor = the largest eligible q_g, +inf when no cell is eligible.
 * 5. Peaks, for k = 0 .. K-1.  g_k = the eligible, not yet excluded cell with the smallest q, ties to the lowest g; the record is
 *    (int32 g_k, int32 0, double q).  Then every cell g with (u_g[0] u_gk[0] + u_g[1] u_gk[1]) + u_g[2] u_gk[2] >= cos_sep, evaluated
 *    in that order, is excluded from the later ranks (g_k itself only if its own product reaches cos_sep: with cos_sep within a
 *    rounding of |u|^2 a cell can take two ranks).  When no cell is left the record is (-1, 0, +inf).
 * 6. Outputs, device memory on 8 bytes.  d_peaks: [n][K] records of 16 bytes; d_floor: double [n]; d_spectrum: NULL, or double [n][G]
 *    holding q_g, ineligible values as computed, a NaN as the quiet NaN 0x7FF8000000000000 (IEEE 754 leaves the sign and the payload
 *    of a computed NaN open).
 * A value outside the ranges above, a table entry that is not finite, n below 0, stride below 1, n or stride or n stride above 2^48, a
 * NULL d_cov, d_peaks or d_floor, a pointer off 8 bytes GACQ_ERR_BAD_ARG.  Everything is checked on the host before anything is
 * launched; a refused call leaves every output untouched; n = 0 does nothing.
 * gacq_bearing_check makes every check that needs no pointer, without a context.  gacq_bearing_open copies the tables to the device
 * (planar) and allocates the workspace (it may wait for the device); gacq_bearing_run_dev is two launches (factors, spectrum and peaks)
 * per chunk of at most min(2^14, 2^24 / G) blocks on the ctx stream, asynchronous, without state between calls and without host
 * synchronisation.  The handle is closed before its context is destroyed.  tests/bearing_oracle.py restates the definition in numpy.
 * ------------------------------------------------------------------------------------------- */
typedef struct gacq_bearing_cfg {
  int antennas;                    /* M, 2..8 */
  int load_shift;                  /* diagonal loading d = (trace >> load_shift) + 1, 0..40 */
  int cells;                       /* G, 1..32768 */
  int peaks;                       /* K, 1..4 */
  double cos_sep;                  /* cells whose direction cosine to a peak reaches this leave the later ranks; -1..1 */
} gacq_bearing_cfg;
typedef struct gacq_bearing gacq_bearing;

int gacq_bearing_check(const gacq_bearing_cfg* cfg, long long n, long long stride);
int gacq_bearing_open(gacq_ctx* ctx, const gacq_bearing_cfg* cfg, const double* a, const double* u, gacq_bearing** out);
int gacq_bearing_run_dev(gacq_bearing* h, const void* d_cov, long long n, long long stride, void* d_peaks, void* d_floor, void* d_spectrum);
void gacq_bearing_close(gacq_bearing* h);

/* ---------------------------------------------------------------------------------------------
 * Navigation data from tracked prompts (gacq_navbits.hip; the framing is host code, gnss_dsp_tools_amd/navdata.py).
 *
 * gacq_navsym: symbol forming and bit synchronisation of K channels, one workgroup per channel.  Everything is host memory: the call
 * uploads, launches one kernel, downloads and returns when the results are there.
 *   prompts: the channels' prompt real parts one after the other, n[k] doubles of channel k (one per 1 ms record);
 *   R[k] in 1..GACQ_NAV_MAX_R records per symbol; overlay[k * GACQ_NAV_MAX_R + r], r < R[k], the +-1 overlay over the records of a symbol;
 *   align: NULL, or per channel -1 (search) or the alignment 0..R-1 to use.
 * For alignment a in 0..R-1 and symbol m, all m with a + (m + 1) R <= n:
 *     S[a][m] = sum_{r = 0..R-1} o[r] p[a + m R + r]      in fp64, r ascending, no fused multiply-add.
 * A non-finite S is an erasure: it is left out of every maximum and sum below and quantises to 0.
 *     e = the binary exponent (frexp) of the largest finite |S[a][m]| of the channel over all a and m (0 when that is 0);
 *     t[a][m] = llrint(ldexp(|S[a][m]|, 40 - e));     E[a] = sum_m t[a][m] in int64 (wrapping; it cannot wrap for n <= 2^23);
 *     a* = the a with the largest E[a], ties to the lowest a, or the caller's;     M = the number of non-erased symbols of a*;
 *     A = ldexp(double(E[a*]) / double(M), e - 40), 0 when M = 0;
 *     q[m] = clamp(rint((S[a*][m] * 48) / A), -127, 127) as int8, 0 when A = 0.  Positive q means bit 0.
 * Results: align_out[k] = a*; E_out[k * GACQ_NAV_MAX_R + a] (0 for a >= R); A_out[k]; nq_out[k] = (n - a*) div R soft symbols of channel
 * k in q_out from offset sum_{i < k} (n[i] div R[i]) (the room of alignment 0).
 * Checked on the host before anything is allocated or launched (gacq_navsym_check makes the same checks and needs no device): K < 1, R
 * outside 1..20, an overlay value other than +-1, align outside -1..R-1, a NULL pointer, n above 2^24 GACQ_ERR_BAD_ARG; n < 2 R - 1 (an
 * alignment without a symbol) GACQ_ERR_SHORT_INPUT.
 *
 * gacq_viterbi_dev: J decodes of the K = 7, rate 1/2 convolutional code, one wave per job, state s in lane s.
 *   Encoder: r[0] the current input bit, r[k] the input k steps before; G1 = 171 (octal) taps r0 r1 r2 r3 r6, G2 = 133 taps r0 r2 r3 r5 r6;
 *   the output order is G1, G2; g2_inverted complements the G2 output.
 *   Trellis: state = the last six inputs, newest in bit 5; input b takes p to ns = (p >> 1) | (b << 5), with r[i] = bit (6 - i) of p;
 *   the predecessors of ns are p0 = (2 ns) & 63 and p1 = p0 | 1.
 *   Metric: coded bit c expects the symbol 1 - 2c; branch metric exp0 q0 + exp1 q1 (int32); path metric max(pm[p0] + bm0, pm[p1] + bm1), a
 *   tie takes p0; no renormalisation (at most 2^20 steps of at most 254 each).  start_state -1: every state starts at 0; otherwise
 *   the other states start at -2^28.  end_state -1: the state with the best metric, ties to the lowest state.
 *   coded[i], i < 2 steps: d_sym[sym_base + i], or with rows > 0 d_sym[sym_base + (i mod rows) cols + i div rows] (rows cols = 2 steps:
 *   the de-interleaver of a block interleaver that is filled column-wise and read row-wise).
 *   Written: d_bits[bit_base + k] = decoded bit first_bit + k, k < nbits (uint8 0 / 1), and d_metric[job] = the metric of the end state.
 * d_sym (int8 [nsym]), d_bits (uint8 [nbits]) and d_metric (int32 [J]) are device memory, jobs is host memory.  One launch on the ctx
 * stream; the call returns after it has finished.  Checked before anything is allocated or launched (gacq_viterbi_check: the same, no
 * device): J < 1, steps outside 1..2^20, a gather that does not hold exactly the job's symbols, a state outside -1..63, a bit range
 * outside the job's steps or the output, a NULL pointer GACQ_ERR_BAD_ARG; symbols outside d_sym GACQ_ERR_SHORT_INPUT.
 * ------------------------------------------------------------------------------------------- */
#define GACQ_NAV_MAX_R 20
typedef struct gacq_vit_job {
  long long sym_base;              /* offset of coded symbol 0 in d_sym */
  long long bit_base;              /* offset in d_bits of the first bit written */
  int steps;                       /* trellis steps, 1..2^20; two symbols each */
  int rows, cols;                  /* gather; rows = 0: none */
  int start_state;                 /* 0..63, or -1: every state starts at 0 */
  int end_state;                   /* 0..63, or -1: the best metric */
  int first_bit, nbits;            /* decoded bits first_bit .. first_bit + nbits - 1 are written */
  int g2_inverted;
} gacq_vit_job;

int gacq_navsym_check(const double* prompts, const int* n, const int* R, const int8_t* overlay, const int* align, int K, const int* align_out,
                      const long long* E_out, const double* A_out, const int8_t* q_out, const int* nq_out);
int gacq_navsym(gacq_ctx* ctx, const double* prompts, const int* n, const int* R, const int8_t* overlay, const int* align, int K,
                int* align_out, long long* E_out, double* A_out, int8_t* q_out, int* nq_out);
int gacq_viterbi_check(const gacq_vit_job* jobs, int J, long long nsym, long long nbits);
int gacq_viterbi_dev(gacq_ctx* ctx, const void* d_sym, long long nsym, const gacq_vit_job* jobs, int J, void* d_bits, long long nbits,
                     void* d_metric);

/* Per-stage GPU time from HIP events recorded on the launch stream (profiling aid for bench.py).
 * Stages: 0 mix/forward, 1 forward FFT (rocFFT), 2 conj-multiply, 3 inverse FFT (rocFFT),
 *         4 magnitude/peak reduce, 5 best-over-Doppler, 6 fused correlate kernel (LDS FFT). */
#define GACQ_NSTAGES 7
int gacq_set_profiling(gacq_ctx* ctx, int enabled);
int gacq_get_stage_time(gacq_ctx* ctx, int stage, double* total_ms, long* launches);
int gacq_reset_stage_times(gacq_ctx* ctx);
const char* gacq_stage_name(int stage);

/* What this device's HBM delivers to a tuned streaming kernel (eight 16-byte non-temporal accesses in flight per lane): kind 0 = fill
 * (stores), 1 = read, 2 = copy (read + write bytes counted), 3 = fill followed by a read of the same buffer (both counted), 4 / 5 / 6 = kinds 0 / 1 / 3 with default-policy instead of non-temporal accesses; `bytes` per launch, `reps` timed launches after two warm-up launches,
 * HIP events on the ctx stream.  The yardstick bench.py holds the HBM-bound kernels against next to the 8 TB/s of the data sheet
 * (roofline.stream_ceiling), measured in the run that reports it.  Synchronous; allocates and frees its own buffers. */
int gacq_stream_probe(gacq_ctx* ctx, int kind, size_t bytes, int reps, double* gbytes_per_s);

/* A HIP stream whose kernels run on a subset of the device's compute units (hipExtStreamCreateWithCUMask; bit b of the mask = logical
 * CU b, which the driver deals round-robin over the XCDs, so the low m bits are m / 8 CUs of every XCD).  For searches of several
 * signals run side by side (the reference runs its PRNs side by side in a Pool, acquire-gps-l1.py:105-108; a cold start searches
 * several signals): the contexts of the memory-bound signals (N = 65536, 61380: Z' round trip through HBM) get a masked stream with
 * gacq_set_stream, the others keep the whole device, and the memory-bound kernels run under the arithmetic of the others
 * (ShardedSearch.search_jobs_async).  The stream is the caller's: destroy it with gacq_stream_destroy after the contexts that used it. */
int gacq_stream_create_cu_mask(int device_id, const uint32_t* cu_mask, int nwords, void** hip_stream_out);
int gacq_stream_destroy(int device_id, void* hip_stream);
/* Where the workgroups of a launch on the ctx stream land: where[i] = xcc_id << 8 | se_id << 5 | sh_id << 4 | cu_id of workgroup i
 * (nworkgroups one-wave workgroups that stay resident 0.2 ms each) -- how tests and tools check what a CU mask selects. */
int gacq_cu_census(gacq_ctx* ctx, int nworkgroups, unsigned* where);

/* Full accumulated magnitude row q[0..N) for one (item, doppler) -- debugging / golden rows. */
int gacq_debug_row(gacq_sig* sig, const float* x_iq, size_t nsamp, int item, double doppler,
                   double bias_hz, int blocks, float* q_out);

/* Table-NCO index vector idx[i] = floor((0 + f*i)*1024) mod 1024, i < N (gnsstools/nco.py:6-9), f = -(bias + doppler)/fs as a
 * search forms it, computed ON THE DEVICE by the forward kernel of the chosen path with the very expression it uses for its
 * table lookup (the kernels are instantiated in a dump mode that stores the index instead of using it).  Index work is
 * bit-exact against the reference; a wrong index moves the metric by less than the 1e-5 tolerance, so it gets its own check.
 * kernel: 1 mix_nco_kernel (rocFFT pipeline), 2 lds_forward_kernel / lds16k_forward_kernel, 3 split_outer_forward_kernel,
 *         4 lds16k_fused_kernel, 5 pfa_outer_forward_kernel.  GACQ_ERR_UNSUPPORTED when that kernel does not serve the signal's N. */
int gacq_debug_nco_indices(gacq_sig* sig, int kernel, double doppler, double bias_hz, int* idx_out);

/* Test hook for "a kernel left a row record undone".  The engines' correlate kernels write one 16-byte record per (epoch, item, bin)
 * into a buffer that lives as long as the context, so a kernel that skips a record leaves whatever the search before it wrote --
 * often the right bytes.  This call overwrites every record of that buffer with one that wins any Doppler scan (peak 1e30, lag 1234,
 * sum 1) and returns how many it wrote (0 before the first search).  row_after >= 0 also arms the next search, once, to overwrite
 * record row_after (index (epoch x items + item) x bins + bin) the same way between its correlate kernels and its Doppler scan:
 * what the results of a search look like when exactly that record was skipped.  -1: nothing armed.  Negative return: error. */
long gacq_debug_poison_rows(gacq_ctx* ctx, long row_after);

/* The block-to-work map of the fused N = 4096 kernel, walked ON THE HOST with the functions the kernel walks with (no device needed):
 * every workgroup of the grid a search of nepoch epochs x nbins Doppler bins x nchunk item chunks would launch with GACQ_OPT_F4K_RUN =
 * run on a device of `cus` compute units, in block order, each workgroup's work items in the order it walks them.
 * info[4] = (resolved run, 1 if the by-epoch map is used, runs per epoch or per XCD, grid size); work[4 i] = (block, epoch, bin, chunk)
 * of the i-th visit, for i < cap.  Returns the number of visits (it may exceed cap), negative on a bad argument.
 * run = -c walks the queues of claimed work (GACQ_OPT_F4K_CLAIM = c) instead: info[4] = (1 if claimed work would be used, by-epoch,
 * 0, grid size), work[4 i] = (queue, epoch, bin, chunk), queue after queue in the order the items are handed out. */
long gacq_debug_f4k_map(int nepoch, int nbins, int nchunk, int run, int cus, int* info, int* work, long cap);

/* Number of rocFFT plans the context has created so far (a plan for a new length costs 0.5-2 s per process: runtime-compiled kernels).
 * The default engines create none -- code spectra included -- for every FFT length of the reference's scripts; the rocFFT pipeline
 * (engine 1), engine 5 outside N = 4096, GACQ_OPT_FUSED_INNER = 0 and gacq_signal_spectrum do, on first use.  Negative: error. */
int gacq_debug_fft_plans(gacq_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* GACQ_H */
