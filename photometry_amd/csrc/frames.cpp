// frames.cpp -- the batched drop-in entry as a native host engine: AperturePhotometry.do_photometry INCLUDING its stamp-resize loop
// (photometry/AperturePhotometry/photometry.py:75-170, BasePhotometry.resize_stamp / _set_stamp BasePhotometry.py:567-693) for every
// target of a CCD region whose frame stacks are resident in HBM, from the target list to columnar results.
//
// What the reference does one target at a time in Python -- cut the stamp out of the HDF5 groups, run the plugin, look at the mask,
// grow the stamp, try again -- is here a JOB: the host submits a batch (tp_frames_submit) and collects it (tp_frames_wait); in
// between a worker thread of the library drives the rounds: group the targets still in play by stamp size, select the catalogue
// stars of every stamp from a cell-binned index, and queue each group's pass on a stream of the engine's pool -- first the halves
// that produce the masks of ALL groups of the round (sum images cropped from the region's, tp_k2p2_masks, the download of what the
// decisions read, an event), then their second halves (extraction, light-curve diagnostics, download of the packed output block
// into page-locked memory).  With the region's TIME-MAJOR stacks at hand (tp_frames_stack.d_images_t ...) nothing is cut: the
// extraction reads a mask pixel's series as one row of the stack (tp_aperture_extract_stack); without them the in-mask rows of
// the stamps are cut per pass (tp_cut_stamps_masked).  The worker then decides with the plugin's rules who is finished, who gets a
// bigger stamp and who gives up.  Small transfers go by a kernel (tp_blit), only the large group's light curves through a DMA
// engine, chunk by chunk on the job's copy stream while the later chunks are still being extracted.  No Python runs between
// submit and collect, so several jobs in flight (one per engine slot) keep the device busy: the first round of one batch runs
// under the latency-bound resize rounds of another.  The rules are those of photometry_amd/stamps.py and plugins.mask_outcome
// (which stay the per-target plugin's implementation and the reference of tests/test_gpu_resize.py); messages travel as codes
// that the Python layer turns into the reference's log strings.  What needs no device -- selection, layouts, planner, decision --
// is in frames_rules.h (checked on the CPU: tests/test_frames_rules_host.py); this file keeps the streams, the memory and the job.
#include "common.h"
#include "frames_rules.h"
#include "helper_pool.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <chrono>
#include <condition_variable>
#include <vector>

namespace fr = frames_rules;

namespace {

constexpr uint32_t kBitmask = 1 | 2 | 4 | 8 | 32 | 64 | 128 | 4096;   // TESSQualityFlags.DEFAULT_BITMASK (quality.py:123-124)
// Streams per job: stream 0 for the large groups, three for the small, latency-bound ones.  Four active streams is what a single
// job runs fastest with (measured, 2 500 targets: 15 / 13 / 20 ms with 2 / 3 / 4 streams for the small groups: beyond four active
// queues of a process the hardware time-slices them).
constexpr int kStreams = 4;               // per slot: three streams of the engine's pool and a copy stream
constexpr int kPoolStreams = kStreams - 1;
constexpr int kFusedFrom = 1024;         // from this many targets on a group is "large": stream 0, the error / background stacks cut after the mask
static_assert(fr::kStatusError == TP_STATUS_ERROR, "frames_rules.h restates the status code");

struct Fail : std::runtime_error { using std::runtime_error::runtime_error; };
inline void ck(tp_ctx* g, int rc) { if (rc != TP_OK) throw Fail(g->err.empty() ? std::string("error ") + std::to_string(rc) : g->err); }
inline void ckh(hipError_t e, const char* what) { if (e != hipSuccess) throw Fail(std::string(what) + ": " + hipGetErrorString(e)); }

// ---- page-locked host memory, pooled by size class (hipHostMalloc takes milliseconds) ---------------------------------------
struct PinnedPool {
	std::mutex m;
	std::multimap<size_t, void*> free_blocks;
	void* get(size_t n, size_t* cap) {
		const size_t c = fr::size_class(n ? n : 16);
		{
			std::lock_guard<std::mutex> lk(m);
			auto it = free_blocks.find(c);
			if (it != free_blocks.end()) { void* p = it->second; free_blocks.erase(it); *cap = c; return p; }
		}
		void* p = nullptr;
		ckh(hipHostMalloc(&p, c, hipHostMallocDefault), "hipHostMalloc");
		*cap = c;
		return p;
	}
	void put(void* p, size_t cap) {
		if (!p) return;
		std::lock_guard<std::mutex> lk(m);
		free_blocks.emplace(cap, p);
	}
	~PinnedPool() { for (auto& kv : free_blocks) (void)hipHostFree(kv.second); }
};

// an event from the pool, or a new one
hipEvent_t take_event(std::vector<hipEvent_t>& event_pool)
{
	if (event_pool.empty()) { hipEvent_t e = nullptr; ckh(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate"); return e; }
	hipEvent_t e = event_pool.back(); event_pool.pop_back();
	return e;
}

// lab (TESSPHOT_FRAMES_TIMING=1): where the worker thread's time goes, microseconds; =11: the queueing of a group step by step as
// well, and when the rounds were queued and decided.  With the variable unset every method returns at once: no clock is read.
struct Timing {
	using clock = std::chrono::steady_clock;
	// catalogue selection + metadata block, queueing a group's device work, waiting for the decisions of a round, deciding, waiting
	// for the last light curves
	enum Slot { SELECT, QUEUE, WAIT, DECIDE, LAST, N_SLOTS };
	bool on = false, detail = false;
	double us[N_SLOTS] = {0, 0, 0, 0, 0};
	int groups = 0, rounds = 0;
	std::map<std::string, double> steps;   // the queueing of a group, step by step
	std::string timeline;                  // when the rounds were queued and decided, microseconds from the start of run()
	clock::time_point run0, prev;
	static double between(clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
	void start() {
		const char* e = std::getenv("TESSPHOT_FRAMES_TIMING");
		on = e && e[0] == '1';
		detail = on && e[1] == '1';
		if (on) run0 = prev = clock::now();
	}
	// now; the laps that follow count from here
	clock::time_point tick() { if (!on) return {}; return prev = clock::now(); }
	// the time since `since` goes to a slot
	clock::time_point add(Slot s, clock::time_point since) { if (!on) return {}; prev = clock::now(); us[s] += between(since, prev); return prev; }
	void lap(const char* what) { if (!detail) return; const auto now = clock::now(); steps[what] += between(prev, now); prev = now; }
	void mark(const char* what, int a, int b) {
		if (!detail) return;
		char buf[96];
		std::snprintf(buf, sizeof buf, " %s%d/%d@%.0f", what, a, b, between(run0, clock::now()));
		timeline += buf;
	}
	void report(int n) const {
		if (!on) return;
		std::fprintf(stderr, "[frames job] %d targets, %d rounds, %d groups: select+metadata %.0f us, queueing %.0f, waiting for decisions %.0f, deciding %.0f, last light curves %.0f\n",
			n, rounds, groups, us[SELECT], us[QUEUE], us[WAIT], us[DECIDE], us[LAST]);
		if (!detail) return;
		std::string line = "[frames job]   queueing:";
		for (auto& kv : steps) { char buf[96]; std::snprintf(buf, sizeof buf, " %s %.0f,", kv.first.c_str(), kv.second); line += buf; }
		std::fprintf(stderr, "%s\n[frames job]   timeline:%s end@%.0f\n", line.c_str(), timeline.c_str(), between(run0, clock::now()));
	}
};

} // namespace

// ---- the catalogue of a region, binned into cells of 16 x 16 pixels (stars sorted by cell) ------------------------------------
struct tp_frames_catalog { fr::CatalogIndex index; };

struct tp_frames_engine {
	int device = 0;
	int n_slots = 0;
	std::vector<tp_ctx*> ctxs;          // kPoolStreams per slot: the engine's pool of streams, shared by the jobs in flight (SmallStream
	                                    // below); the kStreams-th stream of a slot is its copy stream.  The process should stay below
	                                    // ~24 streams in all: beyond that the hardware queues are time-sliced, and with six idle streams
	                                    // more in the process four jobs in flight fell from 8.1 to 4.8 x 10^5 targets/s (round 6)
	// A stream of the pool.  A job's worker CLAIMS one per group of a round while it queues the round (nobody else queues
	// on a claimed stream: a context's host-side state has one user at a time), marks it with an event when it lets go, and the next
	// claimant -- of any job -- prefers a stream whose event has completed (idle), in index order (so that the same few contexts are
	// used and their allocation caches stay warm), else the one with the least work queued since it was last seen idle.
	struct SmallStream { tp_ctx* c = nullptr; hipEvent_t busy = nullptr; double load = 0.0; bool claimed = false; };
	std::vector<SmallStream> small;
	std::mutex sm;
	std::condition_variable released;    // (with sm) claims have been given back
	std::vector<hipStream_t> copy_streams;   // one per slot (nullptr if it could not be created: the light curves then leave on the job's stream)
	std::vector<char> busy;
	std::mutex m;
	PinnedPool pinned;
	HelperPool helpers;
	uint64_t hbm_bytes = 0;
	int running = 0;                     // (with m) worker threads inside run(): tp_frames_engine_destroy waits for them on `idle`
	std::condition_variable idle;
};

namespace {

struct Event { int32_t target, code, a, b; double value; int32_t text; };

struct Group {
	int32_t n = 0, H = 0, W = 0;
	int64_t n_cat = 0, cat_capacity = 1;
	std::vector<int64_t> cat_offsets, cat_starid, target_starid;
	void* h_block = nullptr; size_t h_cap = 0;
	fr::BlockLayout layout;               // of the packed block, on the device and in h_block
};

// a group of one round while its pass is in flight
struct Launched {
	tp_ctx* g = nullptr;
	int small = -1;                       // index of the claimed stream of the engine's pool
	bool chunked = false;                 // its light curves leave on the job's copy stream
	std::vector<int32_t> idx;
	Group grp;
	hipEvent_t ev = nullptr;              // the decisions' data have arrived
	bool failed = false;
	std::string error;
	// what the first half of the pass (metadata, masks, the decisions' download) leaves for the second (cut, extraction, diagnostics)
	std::vector<void*> dev;               // device blocks of this group: freed (stream-ordered) once everything is queued
	tp_cube_desc desc{};
	float* cubes[3] = {nullptr, nullptr, nullptr};
	char* blk = nullptr;
	fr::MetaLayout meta;
	char* d_meta = nullptr;               // the metadata block on the device
	double* d_diag8 = nullptr; int32_t* d_aperture = nullptr;   // scratch of the mask builder
	bool crop = false, large = false, time_major = false;
	template <class T> const T* meta_at(fr::MetaLayout::Field f) const { return meta.at<T>(d_meta, f); }
	template <class T> T* out_at(fr::BlockLayout::Field f) const { return grp.layout.at<T>(blk, f); }
};

// the claims of a round's groups on the pool's streams: they end when the round is queued -- or when anything on the way throws
struct Claims {
	tp_frames_engine* e; std::vector<Launched>& ls; bool held = true;
	void release() {
		if (!held) return;
		held = false;
		std::lock_guard<std::mutex> lk(e->sm);
		for (auto& L : ls) {
			if (L.small < 0) continue;
			auto& S = e->small[(size_t)L.small];
			if (!S.busy) (void)hipEventCreateWithFlags(&S.busy, hipEventDisableTiming);
			if (S.busy) (void)hipEventRecord(S.busy, S.c->stream);
			S.claimed = false;
		}
		e->released.notify_all();
	}
	~Claims() { release(); }
};

} // namespace

struct tp_frames_job {
	tp_frames_engine* eng = nullptr;
	int slot = -1;
	hipStream_t copy_stream = nullptr;        // the slot's copy stream: the light curves of that group, chunk by chunk
	std::vector<hipEvent_t> event_pool;       // events no group holds
	std::vector<hipEvent_t> tails;            // one per group: everything the group queued (its light curves last) has run
	std::vector<std::pair<tp_ctx*, void*>> late_frees;   // output blocks still read by the copy stream when their group was queued
	tp_frames_stack stack{};
	const tp_frames_catalog* cat = nullptr;
	int32_t n = 0, T = 0;
	std::vector<int64_t> starid;
	std::vector<double> tmag, row, col, budget_flux, time;
	std::vector<int64_t> cur;                 // [n][4]
	std::vector<uint8_t> valid;
	std::vector<int32_t> attempts, quality;
	double budget = 0.0;
	// results
	std::vector<int32_t> status, stamp_resizes, group, pos;
	std::vector<uint8_t> has_result;
	std::vector<int64_t> stamp;               // [n][4]
	std::vector<Group> groups;
	std::vector<Event> events;
	std::vector<std::string> texts;
	std::map<int32_t, std::vector<Event>> pending;   // logged, not yet flushed into `events` (plugins._Messages of a target)
	std::vector<std::pair<void*, size_t>> host_scratch;   // pinned metadata blocks: back to the pool when the job is done
	std::thread worker;
	Timing timing;
	int rc = TP_OK;
	std::string err;
	bool joined = false, released = false;
	std::atomic<int> done{0};               // set by the worker when run() has returned (tp_frames_poll)

	void log(int32_t i, int32_t code, int32_t a = 0, int32_t b = 0, double v = 0.0, int32_t text = -1) { pending[i].push_back(Event{i, code, a, b, v, text}); }
	void direct(int32_t i, int32_t code, int32_t a = 0, int32_t b = 0, double v = 0.0, int32_t text = -1) { events.push_back(Event{i, code, a, b, v, text}); }
	void flush(int32_t i) {
		auto it = pending.find(i);
		if (it == pending.end()) return;
		for (auto& e : it->second) events.push_back(e);
		pending.erase(it);
	}
	void finish(int32_t i, int32_t st) {
		status[i] = st;
		for (int k = 0; k < 4; ++k) stamp[(size_t)i * 4 + k] = cur[(size_t)i * 4 + k];
		flush(i);
	}
	int32_t add_text(const std::string& s) { texts.push_back(s); return (int32_t)texts.size() - 1; }
	void* dalloc(Launched& L, size_t nbytes) { void* p = nullptr; ck(L.g, tp_malloc(L.g, nbytes, &p)); L.dev.push_back(p); return p; }
	hipEvent_t tail_event() { tails.push_back(take_event(event_pool)); return tails.back(); }   // (destroyed with the tail events when the job ends)
	void run();
	std::vector<int32_t> start_results();
	std::vector<int32_t> run_round(const std::vector<int32_t>& active);
	void run_part(std::vector<fr::Piece>& part, std::vector<int32_t>& still);
	void settle(Launched& L, std::string& lost, bool& drained, std::vector<int32_t>& still);
	std::string wait_for_tails();
	// the first half of a group's pass, step by step
	void launch_masks(Launched& L);
	fr::Selection select_group(const std::vector<int32_t>& idx);
	Timing::clock::time_point upload_metadata(Launched& L, fr::Selection& sel, Timing::clock::time_point t0);
	void allocate_pass(Launched& L);
	void queue_masks(Launched& L);
	void queue_decisions(Launched& L);
	// ... and the second
	void launch_tail(Launched& L);
	void cut_in_mask_rows(Launched& L);
	int32_t extract(Launched& L, double* const lc[5]);
	void download_tail(Launched& L, int32_t n_chunks);
	void fail_group(Launched& L, const char* what);
	void claim(Launched& L, double work, const std::vector<Launched>& round);
	void drain_all();
	void decide(Launched& L, std::vector<int32_t>& still);
};

// The pass of a group of same-sized stamps on stream L.g, queued in two halves.  launch_masks: metadata upload, the sum images, the
// masks, the download of what the round's decisions read, an event behind it.  launch_tail: the cut of the in-mask rows, the
// extraction, the diagnostics and the download of the light curves, an event behind everything.  The worker queues the first
// halves of ALL groups of a round before any second half: a round is decided from the masks alone, and a mask kernel queued behind
// another group's cut and extraction waited for them (round 6, timeline of a 2 500-target batch: the fourth and fifth group of the
// second round delivered their decisions 2 and 3 ms after the first three).
void tp_frames_job::fail_group(Launched& L, const char* what)
{
	L.failed = true;
	L.error = what;
	if (L.chunked && copy_stream) (void)hipStreamSynchronize(copy_stream);
	(void)hipStreamSynchronize(L.g->stream);
	(void)hipGetLastError();
	for (void* p : L.dev) (void)tp_free(L.g, p);
	L.dev.clear();
	if (L.grp.h_block) { eng->pinned.put(L.grp.h_block, L.grp.h_cap); L.grp.h_block = nullptr; }
	if (L.ev) { event_pool.push_back(L.ev); L.ev = nullptr; }
}

void tp_frames_job::launch_masks(Launched& L)
{
	const auto t0 = timing.tick();
	try {
		Group& G = L.grp;
		G.n = (int32_t)L.idx.size();
		if ((int64_t)G.H * G.W > 32767) throw Fail("a " + std::to_string(G.H) + "x" + std::to_string(G.W) + " stamp is beyond the 32 767 pixels of the mask builder");
		fr::Selection sel = select_group(L.idx);
		const auto t1 = upload_metadata(L, sel, t0);
		allocate_pass(L);
		queue_masks(L);
		queue_decisions(L);
		timing.add(Timing::QUEUE, t1);
		timing.groups += 1;
	} catch (const std::exception& e) {
		const std::string what = e.what();
		fail_group(L, what.c_str());
	}
}

// the catalogue stars of the group's stamps (pipeline._catalogs_of_stamps)
fr::Selection tp_frames_job::select_group(const std::vector<int32_t>& idx)
{
	const size_t m = idx.size();
	if (m < 1024 || eng->helpers.threads.empty()) return fr::select_catalog(cat->index, cur.data(), idx.data(), m);
	// a large group: the stamps in four runs, three of them offered to the engine's helper threads, joined in order.  The
	// selection of 2 500 stamps is 0.5 of the 0.75 ms a worker needs before it can queue anything, 2 of 2.7 ms for 10 000.
	constexpr int K = 4;
	fr::Selection run[K];
	if (!eng->helpers.fork_join(K, [&](int k) {
			const size_t a = m * k / K, b = m * (k + 1) / K;
			run[k] = fr::select_catalog(cat->index, cur.data(), idx.data() + a, b - a);
		}))
		throw Fail("the catalogue selection of the group failed on a helper thread");
	for (int k = 1; k < K; ++k) run[0].append(run[k]);
	return std::move(run[0]);
}

// ---- the metadata of the group as ONE block: one upload.  The group keeps the lists its results are read with.  Returns when the
// block was packed (what comes before is the host's own work, what comes after is queueing)
Timing::clock::time_point tp_frames_job::upload_metadata(Launched& L, fr::Selection& sel, Timing::clock::time_point t0)
{
	using M = fr::MetaLayout;
	Group& G = L.grp;
	const int32_t m = G.n;
	const M& meta = L.meta = M(T, m, sel.n_cat());
	size_t h_cap = 0;
	char* h_meta = static_cast<char*>(eng->pinned.get(meta.nbytes, &h_cap));
	host_scratch.emplace_back(h_meta, h_cap);
	std::memset(h_meta, 0, meta.nbytes);
	auto put = [&](M::Field f, const void* src) { if (meta.size[f]) std::memcpy(h_meta + meta.off[f], src, meta.size[f]); };
	put(M::QUALITY, quality.data()); put(M::TIME, time.data());
	put(M::CAT_OFFSETS, sel.cat_offsets.data()); put(M::CAT_STARID, sel.starid.data()); put(M::CAT_TMAG, sel.tmag.data());
	put(M::CAT_ROW, sel.row.data()); put(M::CAT_COLUMN, sel.col.data());
	put(M::CAT_ROW_STAMP, sel.row_stamp.data()); put(M::CAT_COLUMN_STAMP, sel.col_stamp.data());
	int32_t* stamps32 = meta.at<int32_t>(h_meta, M::STAMPS);
	double* t_row = meta.at<double>(h_meta, M::TARGET_ROW); double* t_col = meta.at<double>(h_meta, M::TARGET_COLUMN);
	double* t_tmag = meta.at<double>(h_meta, M::TARGET_TMAG);
	G.target_starid.resize(m);
	for (int32_t j = 0; j < m; ++j) {
		const int32_t i = L.idx[j];
		for (int k = 0; k < 4; ++k) stamps32[(size_t)j * 4 + k] = (int32_t)cur[(size_t)i * 4 + k];
		t_row[j] = row[i]; t_col[j] = col[i]; t_tmag[j] = tmag[i];
		G.target_starid[j] = starid[i];
	}
	put(M::TARGET_STARID, G.target_starid.data());
	G.n_cat = sel.n_cat();
	G.cat_capacity = G.n_cat > 0 ? G.n_cat : 1;
	G.cat_offsets = std::move(sel.cat_offsets);
	G.cat_starid = std::move(sel.starid);
	const auto t1 = timing.add(Timing::SELECT, t0);
	L.d_meta = static_cast<char*>(dalloc(L, meta.nbytes));
	timing.lap("alloc meta");
	// (measured, TESSPHOT_FRAMES_TIMING: in the first runs of a process this call can return after 8 - 20 ms while other jobs have
	// work queued; in the steady state it takes 30 us.  A kernel that reads the page-locked block through its device mapping never
	// waits, but its system-scope accesses slowed every concurrent kernel: 3.0 x 10^5 targets/s pipelined instead of 5 x 10^5)
	// by a kernel, not by a DMA engine: the streams of a process share the engines, and this upload -- the head of the chain that
	// decides the round -- sat behind the first round's 130 MB of light curves on some streams until THEY had been extracted and
	// copied (round 6, copy trace: the metadata of two of five groups arrived 4 ms late)
	ck(L.g, tp_blit(L.g, L.d_meta, h_meta, meta.nbytes));
	timing.lap("alloc+h2d");
	return t1;
}

// the stamp cubes (where any are needed), the packed output block and the mask builder's scratch
void tp_frames_job::allocate_pass(Launched& L)
{
	tp_ctx* g = L.g;
	Group& G = L.grp;
	const int32_t m = G.n, H = G.H, W = G.W;
	// ---- the three stamp cubes (BasePhotometry._load_cube for the whole group; the cutter writes the padding of the time axis)
	tp_cube_desc& desc = L.desc;
	desc.n_targets = m; desc.n_cad = T; desc.height = H; desc.width = W; desc.t_pitch = fr::round_up(T, 32);
	const size_t cube_bytes = (size_t)m * H * W * (size_t)desc.t_pitch * 4;
	// the region's sum image is at hand (the FFI branch of BasePhotometry.sumimage): no cube is needed before the masks are known
	L.crop = stack.d_sumimage != nullptr;
	// ... and with the time-major stacks no cube is needed at all (launch_tail)
	L.time_major = L.crop && stack.d_images_t != nullptr;
	if (!L.time_major) for (int k = 0; k < 3; ++k) L.cubes[k] = static_cast<float*>(dalloc(L, cube_bytes));
	timing.lap("alloc cubes");
	L.large = m >= kFusedFrom;
	// a small group: one binning of the stamps and one launch for the three stacks.  A large group: the images now, the error and
	// background stacks once the masks are known -- only their in-mask pixel rows are ever read (launch_tail)
	const float* frames[3] = {stack.d_images, stack.d_images_err, stack.d_backgrounds};
	if (!L.crop)
		ck(g, tp_cut_stamps_multi(g, L.large ? 1 : 3, frames, stack.n_frames, stack.n_rows, stack.n_cols, stack.n_cols, (int64_t)stack.n_rows * stack.n_cols,
			stack.row0, stack.col0, L.meta_at<int32_t>(fr::MetaLayout::STAMPS), &desc, L.cubes));
	// ---- the packed output block (comm.packed_block_layout with the catalogue flags, the sum image and the diagnostics)
	G.layout = fr::BlockLayout(m, T, H, W, G.cat_capacity);
	L.blk = static_cast<char*>(dalloc(L, (size_t)G.layout.nbytes));
	ckh(hipMemsetAsync(L.blk, 0, (size_t)G.layout.nbytes, g->stream), "hipMemsetAsync(block)");
	// scratch: the mask builder's diagnostics and the aperture image (bit 1 = collected: every pixel, BasePhotometry.py:1043)
	L.d_diag8 = static_cast<double*>(dalloc(L, (size_t)m * 8 * 8));
	ckh(hipMemsetAsync(L.d_diag8, 0, (size_t)m * 64, g->stream), "hipMemsetAsync(diag)");
	L.d_aperture = static_cast<int32_t*>(dalloc(L, (size_t)m * H * W * 4));
	ckh(hipMemsetAsync(L.d_aperture, 1, (size_t)m * H * W * 4, g->stream), "hipMemsetAsync(aperture)");
	timing.lap("alloc+memsets");
}

// ---- the masks.  The three stand-alone kernels (bit-identical to the fused launch; a small group is latency-bound and spreads
// better over the chip this way).  With the region's sum image: crop, masks, and then (second half) ONE cut of the in-mask rows of
// all three stacks (a sixth of a 15 x 15 stamp: 5.5 GB of traffic per 2 500 stamps instead of 10.8).
void tp_frames_job::queue_masks(Launched& L)
{
	using M = fr::MetaLayout;
	using B = fr::BlockLayout;
	tp_ctx* g = L.g;
	const int32_t m = L.grp.n, H = L.grp.H, W = L.grp.W;
	const int32_t* d_stamps = L.meta_at<int32_t>(M::STAMPS);
	double* d_sum = L.out_at<double>(B::SUMIMAGE);
	if (L.crop) ck(g, tp_crop_sumimage(g, stack.d_sumimage, stack.n_rows, stack.n_cols, stack.n_cols, stack.row0, stack.col0, d_stamps, m, H, W, d_sum));
	else ck(g, tp_sumimage(g, &L.desc, L.cubes[0], L.meta_at<int32_t>(M::QUALITY), 0, kBitmask, nullptr, 0, d_sum));
	timing.lap("crop");
	ck(g, tp_k2p2_masks(g, m, H, W, d_sum, L.meta_at<int64_t>(M::CAT_OFFSETS), L.meta_at<float>(M::CAT_COLUMN_STAMP), L.meta_at<float>(M::CAT_ROW_STAMP),
		L.meta_at<float>(M::CAT_TMAG), L.meta_at<float>(M::CAT_COLUMN), L.meta_at<float>(M::CAT_ROW), L.meta_at<int64_t>(M::CAT_STARID),
		L.meta_at<double>(M::TARGET_ROW), L.meta_at<double>(M::TARGET_COLUMN), L.meta_at<double>(M::TARGET_TMAG), L.meta_at<int64_t>(M::TARGET_STARID),
		d_stamps, L.d_aperture, nullptr, nullptr, L.out_at<uint8_t>(B::MASK), L.out_at<int32_t>(B::STATUS), L.out_at<int32_t>(B::FLAGS),
		L.out_at<double>(B::CONTAMINATION), L.d_diag8, L.out_at<uint8_t>(B::CAT_IN_MASK)));
	timing.lap("k2p2");
}

// ---- downloads: what the decisions read (status, flags, mask, catalogue flags, sum image) is complete once the masks are --
// it leaves now, with an event, and the worker decides the job's next round while this group's extraction and diagnostics run
// (nothing of a round is decided from the light curves; a target that is cut again has its extraction redone anyway)
void tp_frames_job::queue_decisions(Launched& L)
{
	Group& G = L.grp;
	const fr::BlockLayout& B = G.layout;
	G.h_block = eng->pinned.get((size_t)B.nbytes, &G.h_cap);
	timing.lap("pinned");
	const uint64_t from = B.off[B.CONTAMINATION];
	ck(L.g, tp_blit(L.g, static_cast<char*>(G.h_block) + from, L.blk + from, B.off[B.DIAGNOSTICS] - from));   // (by a kernel: see the metadata)
	L.ev = take_event(event_pool);
	ckh(hipEventRecord(L.ev, L.g->stream), "hipEventRecord");
	timing.lap("d2h+event");
}

void tp_frames_job::launch_tail(Launched& L)
{
	if (L.failed) return;
	using B = fr::BlockLayout;
	tp_ctx* g = L.g;
	const int32_t m = L.grp.n;
	const auto t1 = timing.tick();
	try {
		cut_in_mask_rows(L);
		timing.lap("masked cut");
		double* lc[5];
		for (int k = 0; k < 5; ++k) lc[k] = L.out_at<double>(B::LC) + (size_t)k * m * T;
		const int32_t n_chunks = extract(L, lc);
		timing.lap("extract");
		ck(g, tp_lightcurve_diagnostics(g, m, T, lc[0], lc[1], lc[3], lc[4], T, L.meta_at<double>(fr::MetaLayout::TIME), L.meta_at<int32_t>(fr::MetaLayout::QUALITY),
			0, kBitmask, L.out_at<int32_t>(B::STATUS), L.out_at<double>(B::SUMIMAGE), L.out_at<uint8_t>(B::MASK), L.grp.H, L.grp.W, 3600.0 / 86400.0,
			L.out_at<double>(B::DIAGNOSTICS)));
		timing.lap("diagnostics");
		download_tail(L, n_chunks);
		timing.lap("d2h light curves");
		// the group's last word: the job ends when the tail events of all its groups have completed (its streams are shared)
		ckh(hipEventRecord(tail_event(), g->stream), "hipEventRecord");
		for (void* p : L.dev) (void)tp_free(g, p);      // stream-ordered: handed out again only after what is queued above has run
		L.dev.clear();
		timing.add(Timing::QUEUE, t1);
	} catch (const std::exception& e) {
		// (the round's decisions are taken after both halves of all its groups have been queued: the group counts as failed, as if
		// its first half had)
		const std::string what = e.what();
		fail_group(L, what.c_str());
	}
}

// For a large group the cut of the error and background stacks comes BETWEEN mask and extraction and writes in-mask rows only:
// of 8.9 GB of cubes per 2 500 stamps of 15 x 15 the passes read 4.4 (the images for the sum image, a sixth of the rows of all
// three for the extraction), so two thirds of the old cut's writes were never read
void tp_frames_job::cut_in_mask_rows(Launched& L)
{
	if (L.time_major) return;     // nothing to cut: the extraction reads the rows of the time-major stacks
	const float* frames[3] = {stack.d_images, stack.d_images_err, stack.d_backgrounds};
	const int first = L.crop ? 0 : 1;      // (without the region's sum image the images were cut for the group's own)
	if (L.crop || L.large)
		ck(L.g, tp_cut_stamps_masked(L.g, 3 - first, frames + first, stack.n_frames, stack.n_rows, stack.n_cols, stack.n_cols, (int64_t)stack.n_rows * stack.n_cols,
			stack.row0, stack.col0, L.meta_at<int32_t>(fr::MetaLayout::STAMPS), &L.desc, L.out_at<uint8_t>(fr::BlockLayout::MASK), L.cubes + first));
}

// The light curves of a large group are most of what the call downloads (130 MB per 2 500 targets: 2.3 ms of the link), and they
// used to leave when extraction AND diagnostics of the whole group were done.  Now the group is extracted in chunks of targets,
// and a chunk's five planes leave on the job's copy stream as soon as the chunk is extracted: the link starts 0.15 ms after the
// cut instead of 1.2 ms, and the diagnostics run under the copies.  Returns the number of chunks.
int32_t tp_frames_job::extract(Launched& L, double* const lc[5])
{
	tp_ctx* g = L.g;
	const Group& G = L.grp;
	const int32_t m = G.n, H = G.H, W = G.W;
	const int32_t* d_stamps = L.meta_at<int32_t>(fr::MetaLayout::STAMPS);
	const int32_t* d_status = L.out_at<int32_t>(fr::BlockLayout::STATUS);
	const uint8_t* d_mask = L.out_at<uint8_t>(fr::BlockLayout::MASK);
	const int32_t n_chunks = (copy_stream && m >= 2048) ? std::min<int32_t>(8, m / 512) : 1;
	L.chunked = n_chunks > 1;
	for (int32_t c = 0; c < n_chunks; ++c) {
		const int32_t j0 = (int32_t)((int64_t)m * c / n_chunks), j1 = (int32_t)((int64_t)m * (c + 1) / n_chunks);
		tp_cube_desc part = L.desc;
		part.n_targets = j1 - j0;
		const size_t cube_off = (size_t)j0 * H * W * (size_t)L.desc.t_pitch;
		if (L.time_major)
			ck(g, tp_aperture_extract_stack(g, j1 - j0, T, H, W, stack.d_images_t, stack.d_images_err_t, stack.d_backgrounds_t, stack.t_pitch,
				stack.n_rows, stack.n_cols, stack.row0, stack.col0,
				d_mask + (size_t)j0 * H * W, d_stamps + (size_t)j0 * 4, d_status + j0,
				lc[0] + (size_t)j0 * T, lc[1] + (size_t)j0 * T, lc[2] + (size_t)j0 * T, lc[3] + (size_t)j0 * T, lc[4] + (size_t)j0 * T, T));
		else
			ck(g, tp_aperture_extract(g, &part, L.cubes[0] + cube_off, L.cubes[1] + cube_off, L.cubes[2] + cube_off, 0, 0, nullptr, 0,
				d_mask + (size_t)j0 * H * W, d_stamps + (size_t)j0 * 4, d_status + j0,
				lc[0] + (size_t)j0 * T, lc[1] + (size_t)j0 * T, lc[2] + (size_t)j0 * T, lc[3] + (size_t)j0 * T, lc[4] + (size_t)j0 * T, T));
		if (n_chunks > 1) {
			hipEvent_t e = tail_event();
			ckh(hipEventRecord(e, g->stream), "hipEventRecord");
			ckh(hipStreamWaitEvent(copy_stream, e, 0), "hipStreamWaitEvent");
			// the five planes of the chunk as ONE rectangular copy (five rows, a plane apart): 48 DMA commands per 2 500 targets instead
			// of 240, each followed by ~20 us of idle link (copy trace of four jobs in flight: the link was busy 87 % of the time;
			// 7.55 -> 7.98 x 10^5 targets/s)
			const size_t o = (size_t)G.layout.off[fr::BlockLayout::LC] + (size_t)j0 * T * 8;
			ckh(hipMemcpy2DAsync(static_cast<char*>(G.h_block) + o, (size_t)m * T * 8, L.blk + o, (size_t)m * T * 8, (size_t)(j1 - j0) * T * 8, 5,
				hipMemcpyDeviceToHost, copy_stream), "hipMemcpy2DAsync(light curves)");
		}
	}
	return n_chunks;
}

// the diagnostics, and the light curves unless they have left in chunks
void tp_frames_job::download_tail(Launched& L, int32_t n_chunks)
{
	tp_ctx* g = L.g;
	const Group& G = L.grp;
	const fr::BlockLayout& B = G.layout;
	char* blk = L.blk;
	const uint64_t lc_bytes = B.off[B.CONTAMINATION], off_diag = B.off[B.DIAGNOSTICS];
	// (by a kernel, like everything but the large group's light curves: a copy that waits in a DMA engine's queue behind another
	// job's 130 MB holds this STREAM, and the next round's masks queued on it, for as long)
	ck(g, tp_blit(g, static_cast<char*>(G.h_block) + off_diag, blk + off_diag, B.nbytes - off_diag));
	if (n_chunks > 1) {
		// the copies' end is one of the job's tail events.  The group's stream does NOT wait for them (it would be held, and whatever
		// another job queues on it next, for the 2 - 10 ms the link takes): the output block they read is the one block of the group
		// that is not given back in stream order below -- it goes back when the job has seen its tail events
		ckh(hipEventRecord(tail_event(), copy_stream), "hipEventRecord");
		for (size_t i = 0; i < L.dev.size(); ++i)
			if (L.dev[i] == static_cast<void*>(blk)) { L.dev.erase(L.dev.begin() + (long)i); late_frees.emplace_back(g, static_cast<void*>(blk)); break; }
	} else if (lc_bytes <= ((uint64_t)32 << 20)) {
		ck(g, tp_blit(g, G.h_block, blk, lc_bytes));
	} else {
		ckh(hipMemcpyAsync(G.h_block, blk, (size_t)lc_bytes, hipMemcpyDeviceToHost, g->stream), "hipMemcpyAsync(light curves)");
	}
}

// the plugin's rules on the results of one group (fr::decide_target), and the job's bookkeeping of what they say
void tp_frames_job::decide(Launched& L, std::vector<int32_t>& still)
{
	using B = fr::BlockLayout;
	Group& G = L.grp;
	const int32_t m = G.n, H = G.H, W = G.W;
	const int32_t gid = (int32_t)groups.size();
	const int32_t* r_status = G.layout.at<int32_t>(G.h_block, B::STATUS);
	const int32_t* r_flags = G.layout.at<int32_t>(G.h_block, B::FLAGS);
	const uint8_t* r_mask = G.layout.at<uint8_t>(G.h_block, B::MASK);
	const double* r_sum = G.layout.at<double>(G.h_block, B::SUMIMAGE);
	for (int32_t j = 0; j < m; ++j) {
		const int32_t i = L.idx[j];
		int64_t* st = &cur[(size_t)i * 4];
		const fr::Attempt t{r_flags[j], r_status[j], {st[0], st[1], st[2], st[3]},
			{stack.row0, (int64_t)stack.row0 + stack.n_rows, stack.col0, (int64_t)stack.col0 + stack.n_cols},
			attempts[i], budget_flux[i], r_mask + (size_t)j * H * W, r_sum + (size_t)j * H * W, H, W};
		attempts[i] -= 1;
		const fr::Decision d = fr::decide_target(t);
		for (int k = 0; k < d.n_codes; ++k) {
			if (d.codes[k] == 5) direct(i, 5, d.kind);
			else log(i, d.codes[k], 0, 0, d.codes[k] == 7 ? d.edge_flux : 0.0);
		}
		if (d.moved) {
			stamp_resizes[i] += 1;
			for (int k = 0; k < 4; ++k) st[k] = d.stamp[k];
		}
		if (d.outcome == fr::Decision::RESIZE) { still.push_back(i); continue; }
		if (d.outcome == fr::Decision::STANDS) { has_result[i] = 1; group[i] = gid; pos[i] = j; }
		finish(i, d.status);
	}
	groups.push_back(std::move(G));
}

// a stream of the engine's pool for a small group: an idle one (its last claimant's event has completed) in index order, else the one
// with the least work queued since it was last seen idle; claimed until the round is queued
void tp_frames_job::claim(Launched& L, double work, const std::vector<Launched>& round)
{
	std::unique_lock<std::mutex> lk(eng->sm);
	for (;;) {
		int pick = -1;
		for (size_t k = 0; k < eng->small.size(); ++k) {
			auto& S = eng->small[k];
			if (S.claimed) continue;
			if (S.busy && S.load > 0.0 && hipEventQuery(S.busy) == hipSuccess) S.load = 0.0;   // drained
			if (S.load == 0.0) { pick = (int)k; break; }
			if (pick < 0 || S.load < eng->small[(size_t)pick].load) pick = (int)k;
		}
		(void)hipGetLastError();   // hipErrorNotReady of the queries
		if (pick < 0)                // none unclaimed.  A round with more groups than the pool has streams: one this job holds already
			for (const Launched& o : round)
				if (o.small >= 0 && (pick < 0 || eng->small[(size_t)o.small].load < eng->small[(size_t)pick].load)) pick = o.small;
		if (pick >= 0) {
			auto& S = eng->small[(size_t)pick];
			S.claimed = true;
			S.load += work;
			L.small = pick;
			L.g = S.c;
			return;
		}
		eng->released.wait(lk);      // every stream of the pool is claimed by other jobs' workers until they have queued their rounds
	}
}

// error paths: everything this job may have queued anywhere has run (its copy stream and the whole pool)
void tp_frames_job::drain_all()
{
	if (copy_stream) (void)hipStreamSynchronize(copy_stream);
	for (auto& S : eng->small) (void)hipStreamSynchronize(S.c->stream);
	(void)hipGetLastError();
}

// the result arrays, and the targets that take part
std::vector<int32_t> tp_frames_job::start_results()
{
	status.assign(n, 0); stamp_resizes.assign(n, 0); group.assign(n, -1); pos.assign(n, 0); has_result.assign(n, 0);
	stamp.assign((size_t)n * 4, -1);
	std::vector<int32_t> active;
	for (int32_t i = 0; i < n; ++i) {
		if (valid[i]) { active.push_back(i); continue; }
		status[i] = TP_STATUS_ERROR;                    // BasePhotometry.py:671-672: the constructor raises
		direct(i, 12);
		stamp[(size_t)i * 4] = -1; stamp[(size_t)i * 4 + 1] = -2; stamp[(size_t)i * 4 + 2] = -1; stamp[(size_t)i * 4 + 3] = -2;
	}
	return active;
}

void tp_frames_job::run()
{
	(void)hipSetDevice(eng->device);
	timing.start();
	try {
		std::vector<int32_t> active = start_results();
		while (!active.empty()) active = run_round(active);
		const std::string copy_error = wait_for_tails();
		timing.report((int)n);
		if (!copy_error.empty()) {       // nothing that was extracted can be trusted
			const int32_t t = add_text(copy_error);
			for (int32_t i = 0; i < n; ++i) if (has_result[i]) { has_result[i] = 0; direct(i, 11, 0, 0, 0.0, t); status[i] = TP_STATUS_ERROR; }
		}
	} catch (const std::exception& e) {
		rc = TP_ERR_HIP;
		err = e.what();
		drain_all();
		for (auto& lf : late_frees) (void)tp_free(lf.first, lf.second);
		late_frees.clear();
	}
	for (auto e : tails) (void)hipEventDestroy(e);
	tails.clear();
	for (auto e : event_pool) (void)hipEventDestroy(e);
	event_pool.clear();
	for (auto& hs : host_scratch) eng->pinned.put(hs.first, hs.second);
	host_scratch.clear();
}

// one round: the groups of the targets in play (fr::plan_round), part by part; returns the targets that go on with a larger stamp
std::vector<int32_t> tp_frames_job::run_round(const std::vector<int32_t>& active)
{
	auto parts = fr::plan_round(active, cur.data(), T, !(stack.d_sumimage && stack.d_images_t), budget);
	std::vector<int32_t> still;
	for (auto& part : parts) run_part(part, still);
	std::sort(still.begin(), still.end());
	return still;
}

// the groups that run side by side: both halves of every pass queued, then decided one by one as their masks arrive
void tp_frames_job::run_part(std::vector<fr::Piece>& part, std::vector<int32_t>& still)
{
	std::vector<Launched> launched(part.size());
	Claims claims{eng, launched};
	for (size_t gi = 0; gi < part.size(); ++gi) {
		Launched& L = launched[gi];
		L.idx = std::move(part[gi].idx);
		L.grp.H = part[gi].H; L.grp.W = part[gi].W;
		// Every group takes a stream of the engine's pool, an IDLE one if there is one: the large group of the first round as
		// well as the resized stamps of a few targets -- chains of latency-bound launches that decide when the job's next
		// round can start.  Until round 6 a job had four streams of its own, three of them for the small groups, taken in
		// turn: the fourth and fifth group of a round queued behind the first two's cut, extraction and diagnostics, and a
		// round of five groups was decided 3 ms after its first three masks were done.  (More streams per JOB do not help:
		// with 7 per job, 35 in the engine, a call alone took 11 - 14 ms instead of 7.6 -- see the note at the pool.)
		const double work = (double)L.idx.size() * (double)L.grp.H * (double)L.grp.W;   // what its tail costs, roughly
		claim(L, work, launched);
	}
	for (auto& L : launched) launch_masks(L);
	for (auto& L : launched) launch_tail(L);
	claims.release();
	timing.rounds += 1;
	timing.mark("queued", timing.rounds, (int)launched.size());
	std::string lost;                        // a device error that surfaces at an event costs every group of the part
	bool drained = false;                    // ... and the job's streams are drained once before any of its blocks is given back
	for (auto& L : launched) settle(L, lost, drained, still);
}

// wait for a group's masks and decide its targets; a group that failed, or any group once the device is lost, ends its targets in error
void tp_frames_job::settle(Launched& L, std::string& lost, bool& drained, std::vector<int32_t>& still)
{
	const auto a = timing.tick();
	if (!L.failed && lost.empty()) {
		const hipError_t e = hipEventSynchronize(L.ev);
		if (e != hipSuccess) { lost = std::string("hipEventSynchronize: ") + hipGetErrorString(e); (void)hipGetLastError(); }
	}
	const auto b = timing.add(Timing::WAIT, a);
	timing.mark("ev", timing.rounds, (int)L.idx.size());
	if (L.ev) { event_pool.push_back(L.ev); L.ev = nullptr; }
	if (L.failed || !lost.empty()) {
		// the copies into this part's page-locked blocks may still be queued (on this group's stream, or -- once an error
		// has surfaced and the remaining groups are no longer waited for one by one -- on any of the job's streams): a block
		// goes back to the engine-wide pool, where another job's thread may take it, only after they have drained
		if (!drained) { drain_all(); drained = true; }
		if (L.grp.h_block) { eng->pinned.put(L.grp.h_block, L.grp.h_cap); L.grp.h_block = nullptr; }
		const int32_t t = add_text(L.failed ? L.error : lost);
		for (int32_t i : L.idx) { log(i, 10, L.grp.H, L.grp.W, 0.0, t); finish(i, TP_STATUS_ERROR); }
	} else decide(L, still);
	timing.add(Timing::DECIDE, b);
}

// ---- the light curves of every round have arrived; returns the first error of a copy, if any
std::string tp_frames_job::wait_for_tails()
{
	std::string copy_error;
	const auto w = timing.tick();
	for (hipEvent_t te : tails) {
		const hipError_t e = hipEventSynchronize(te);
		if (e != hipSuccess && copy_error.empty()) { copy_error = std::string("hipEventSynchronize: ") + hipGetErrorString(e); (void)hipGetLastError(); }
	}
	for (auto& lf : late_frees) (void)tp_free(lf.first, lf.second);   // (the allocator of a context is serialised by its own mutex)
	late_frees.clear();
	timing.add(Timing::LAST, w);
	return copy_error;
}

extern "C" {

int tp_frames_engine_create(int device, int32_t n_slots, tp_frames_engine** out)
{
	if (!out) { tp_global_err = "tp_frames_engine_create: null output pointer"; return TP_ERR_INVALID; }
	*out = nullptr;
	if (n_slots < 1 || n_slots > 64) { tp_global_err = "tp_frames_engine_create: 1 .. 64 slots"; return TP_ERR_INVALID; }
	TP_API_BEGIN
	tp_frames_engine* eng = new tp_frames_engine();
	eng->device = device;
	eng->n_slots = n_slots;
	for (int i = 0; i < n_slots * kPoolStreams; ++i) {
		tp_ctx* c = nullptr;
		const int rc = tp_ctx_create_stream(device, 0, &c);
		if (rc != TP_OK) {
			for (tp_ctx* x : eng->ctxs) (void)tp_ctx_destroy(x);
			delete eng;
			return rc;
		}
		c->reuse_in_stream_order = true;      // (every block of a group is allocated from, used on and freed to the context of its stream)
		eng->ctxs.push_back(c);
		tp_frames_engine::SmallStream S; S.c = c; eng->small.push_back(S);
	}
	eng->busy.assign(n_slots, 0);
	eng->helpers.start(3);
	eng->copy_streams.assign(n_slots, nullptr);
	(void)hipSetDevice(device);
	for (int i = 0; i < n_slots; ++i)
		if (hipStreamCreateWithFlags(&eng->copy_streams[(size_t)i], hipStreamNonBlocking) != hipSuccess) { eng->copy_streams[(size_t)i] = nullptr; (void)hipGetLastError(); }
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) eng->hbm_bytes = (uint64_t)prop.totalGlobalMem;
	*out = eng;
	return TP_OK;
	TP_API_END((tp_ctx*)nullptr)
}

int tp_frames_engine_destroy(tp_frames_engine* eng)
{
	if (!eng) return TP_OK;
	{                                // (a job still running: its streams go only once it is through)
		std::unique_lock<std::mutex> lk(eng->m);
		eng->idle.wait(lk, [eng] { return eng->running == 0; });
	}
	for (auto& S : eng->small) if (S.busy) (void)hipEventDestroy(S.busy);
	for (hipStream_t cs : eng->copy_streams) if (cs) (void)hipStreamDestroy(cs);
	for (tp_ctx* c : eng->ctxs) (void)tp_ctx_destroy(c);
	delete eng;
	return TP_OK;
}

int tp_frames_engine_info(tp_frames_engine* eng, int32_t* n_slots, int32_t* n_free, uint64_t* hbm_bytes)
{
	if (!eng) { tp_global_err = "null engine"; return TP_ERR_INVALID; }
	std::lock_guard<std::mutex> lk(eng->m);
	if (n_slots) *n_slots = eng->n_slots;
	if (n_free) { int f = 0; for (char b : eng->busy) f += b ? 0 : 1; *n_free = f; }
	if (hbm_bytes) *hbm_bytes = eng->hbm_bytes;
	return TP_OK;
}

int tp_frames_catalog_create(int64_t n_stars, const int64_t* h_starid, const float* h_tmag, const double* h_row, const double* h_column,
	tp_frames_catalog** out)
{
	if (!out || n_stars < 0 || (n_stars > 0 && !(h_starid && h_tmag && h_row && h_column))) { tp_global_err = "tp_frames_catalog_create: bad arguments"; return TP_ERR_INVALID; }
	*out = nullptr;
	TP_API_BEGIN
	tp_frames_catalog* c = new tp_frames_catalog();
	c->index.build(n_stars, h_starid, h_tmag, h_row, h_column);
	*out = c;
	return TP_OK;
	TP_API_END((tp_ctx*)nullptr)
}

int tp_frames_catalog_destroy(tp_frames_catalog* cat)
{
	delete cat;
	return TP_OK;
}

int tp_frames_submit(tp_frames_engine* eng, const tp_frames_stack* stack, const tp_frames_catalog* cat,
	int32_t n_targets, const int64_t* h_starid, const double* h_tmag, const double* h_row, const double* h_column,
	const int64_t* h_stamps, const uint8_t* h_valid, const int32_t* h_attempts, const double* h_quick_break_budget,
	const double* h_time, const int32_t* h_quality, double budget_bytes, tp_frames_job** out)
{
	if (!eng || !out) { tp_global_err = "tp_frames_submit: null engine / output pointer"; return TP_ERR_INVALID; }
	*out = nullptr;
	if (!stack || !cat || n_targets < 0 || !stack->d_images || !stack->d_images_err || !stack->d_backgrounds || stack->n_frames <= 0 ||
		stack->n_rows <= 0 || stack->n_cols <= 0 || !h_time || !h_quality ||
		(n_targets > 0 && !(h_starid && h_tmag && h_row && h_column && h_stamps && h_valid && h_attempts && h_quick_break_budget))) {
		tp_global_err = "tp_frames_submit: bad arguments";
		return TP_ERR_INVALID;
	}
	if (stack->d_images_t || stack->d_images_err_t || stack->d_backgrounds_t) {
		if (!(stack->d_images_t && stack->d_images_err_t && stack->d_backgrounds_t && stack->d_sumimage) || stack->t_pitch < stack->n_frames || stack->t_pitch % 4 != 0 ||
			(int64_t)stack->n_rows * stack->n_cols >= ((int64_t)1 << 31)) {
			tp_global_err = "tp_frames_submit: the time-major stacks come all three, with the region's sum image, and t_pitch >= n_frames, a multiple of 4";
			return TP_ERR_INVALID;
		}
	}
	TP_API_BEGIN
	int slot = -1;
	{
		std::lock_guard<std::mutex> lk(eng->m);
		for (int s = 0; s < eng->n_slots; ++s) if (!eng->busy[s]) { slot = s; eng->busy[s] = 1; break; }
	}
	if (slot < 0) { tp_global_err = "tp_frames_submit: every slot of the engine holds a job (wait for and release one first)"; return TP_ERR_INVALID; }
	tp_frames_job* job = new tp_frames_job();
	job->eng = eng; job->slot = slot;
	job->copy_stream = eng->copy_streams[(size_t)slot];
	job->stack = *stack; job->cat = cat;
	job->n = n_targets; job->T = stack->n_frames;
	job->starid.assign(h_starid, h_starid + n_targets);
	job->tmag.assign(h_tmag, h_tmag + n_targets);
	job->row.assign(h_row, h_row + n_targets);
	job->col.assign(h_column, h_column + n_targets);
	job->cur.assign(h_stamps, h_stamps + (size_t)n_targets * 4);
	job->valid.assign(h_valid, h_valid + n_targets);
	job->attempts.assign(h_attempts, h_attempts + n_targets);
	job->budget_flux.assign(h_quick_break_budget, h_quick_break_budget + n_targets);
	job->time.assign(h_time, h_time + job->T);
	job->quality.assign(h_quality, h_quality + job->T);
	job->budget = budget_bytes > 0 ? budget_bytes : (double)eng->hbm_bytes / 4.0;
	{ std::lock_guard<std::mutex> lk(eng->m); eng->running += 1; }
	try {
		job->worker = std::thread([job] {
			job->run();
			job->done.store(1, std::memory_order_release);
			tp_frames_engine* e = job->eng;
			std::lock_guard<std::mutex> lk(e->m);   // (notified under the lock: the engine may go as soon as it is released)
			e->running -= 1;
			e->idle.notify_all();
		});
	} catch (...) {          // no thread to be had: the slot is free again, the job never existed
		{ std::lock_guard<std::mutex> lk(eng->m); eng->busy[slot] = 0; eng->running -= 1; }
		delete job;
		tp_global_err = "tp_frames_submit: could not start the job's worker thread";
		return TP_ERR_INVALID;
	}
	*out = job;
	return TP_OK;
	TP_API_END((tp_ctx*)nullptr)
}

int tp_frames_wait(tp_frames_job* job)
{
	if (!job) { tp_global_err = "null job"; return TP_ERR_INVALID; }
	if (!job->joined) {
		job->worker.join();
		job->joined = true;
		// the job's streams are idle: its slot can take the next job while the caller still holds this one's results
		std::lock_guard<std::mutex> lk(job->eng->m);
		job->eng->busy[job->slot] = 0;
	}
	if (job->rc != TP_OK) tp_global_err = job->err;
	return job->rc;
}

int tp_frames_poll(tp_frames_job* job, int32_t* done)
{
	if (!job || !done) { tp_global_err = "tp_frames_poll: null pointer"; return TP_ERR_INVALID; }
	*done = (job->joined || job->done.load(std::memory_order_acquire)) ? 1 : 0;
	return TP_OK;
}

int tp_frames_counts(tp_frames_job* job, int32_t* n_groups, int64_t* n_events)
{
	if (!job || !job->joined) { tp_global_err = "tp_frames_counts: wait for the job first"; return TP_ERR_INVALID; }
	if (n_groups) *n_groups = (int32_t)job->groups.size();
	if (n_events) *n_events = (int64_t)job->events.size();
	return TP_OK;
}

int tp_frames_targets(tp_frames_job* job, int32_t* status, int64_t* stamps, int32_t* stamp_resizes, uint8_t* has_result, int32_t* group, int32_t* pos)
{
	if (!job || !job->joined) { tp_global_err = "tp_frames_targets: wait for the job first"; return TP_ERR_INVALID; }
	const size_t n = (size_t)job->n;
	if (status) std::memcpy(status, job->status.data(), n * 4);
	if (stamps) std::memcpy(stamps, job->stamp.data(), n * 32);
	if (stamp_resizes) std::memcpy(stamp_resizes, job->stamp_resizes.data(), n * 4);
	if (has_result) std::memcpy(has_result, job->has_result.data(), n);
	if (group) std::memcpy(group, job->group.data(), n * 4);
	if (pos) std::memcpy(pos, job->pos.data(), n * 4);
	return TP_OK;
}

int tp_frames_group(tp_frames_job* job, int32_t g, int32_t* n_targets, int32_t* height, int32_t* width, int64_t* cat_capacity, int64_t* n_cat,
	void** h_block, uint64_t* block_nbytes)
{
	if (!job || !job->joined || g < 0 || g >= (int32_t)job->groups.size()) { tp_global_err = "tp_frames_group: no such group"; return TP_ERR_INVALID; }
	const Group& G = job->groups[g];
	if (n_targets) *n_targets = G.n;
	if (height) *height = G.H;
	if (width) *width = G.W;
	if (cat_capacity) *cat_capacity = G.cat_capacity;
	if (n_cat) *n_cat = G.n_cat;
	if (h_block) *h_block = G.h_block;
	if (block_nbytes) *block_nbytes = G.layout.nbytes;
	return TP_OK;
}

int tp_frames_group_lists(tp_frames_job* job, int32_t g, int64_t* cat_offsets, int64_t* cat_starid, int64_t* target_starid)
{
	if (!job || !job->joined || g < 0 || g >= (int32_t)job->groups.size()) { tp_global_err = "tp_frames_group_lists: no such group"; return TP_ERR_INVALID; }
	const Group& G = job->groups[g];
	if (cat_offsets) std::memcpy(cat_offsets, G.cat_offsets.data(), G.cat_offsets.size() * 8);
	if (cat_starid && G.n_cat) std::memcpy(cat_starid, G.cat_starid.data(), (size_t)G.n_cat * 8);
	if (target_starid) std::memcpy(target_starid, G.target_starid.data(), (size_t)G.n * 8);
	return TP_OK;
}

int tp_frames_events(tp_frames_job* job, int32_t* target, int32_t* code, int32_t* a, int32_t* b, double* value, int32_t* text)
{
	if (!job || !job->joined) { tp_global_err = "tp_frames_events: wait for the job first"; return TP_ERR_INVALID; }
	for (size_t k = 0; k < job->events.size(); ++k) {
		const Event& e = job->events[k];
		if (target) target[k] = e.target;
		if (code) code[k] = e.code;
		if (a) a[k] = e.a;
		if (b) b[k] = e.b;
		if (value) value[k] = e.value;
		if (text) text[k] = e.text;
	}
	return TP_OK;
}

const char* tp_frames_text(tp_frames_job* job, int32_t k)
{
	if (!job || k < 0 || k >= (int32_t)job->texts.size()) return "";
	return job->texts[k].c_str();
}

int tp_frames_release(tp_frames_job* job)
{
	if (!job) return TP_OK;
	(void)tp_frames_wait(job);
	for (auto& G : job->groups) if (G.h_block) { job->eng->pinned.put(G.h_block, G.h_cap); G.h_block = nullptr; }
	delete job;
	return TP_OK;
}

} // extern "C"
