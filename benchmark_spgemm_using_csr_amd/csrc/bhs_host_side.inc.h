// bhs_host_side.inc.h -- what the operations beside the multiply pipeline share on the host: the masked and the semiring
// multiply, the sparse add, the entry selection, the transpose, the extraction, the reductions and the scaling, CSR x dense,
// the assembly, and the graph and solver calls
// (A part of bhsparse_hip.hip's translation unit: included there inside its unnamed namespace, ahead of the pipeline, whose
// scan takes its epochs from here too; the control words it names are those of bhs_aggregate.hip.h, which the unit includes
// with its other device headers.)
//
// Every family keeps a workspace of its own on the handle (SideWs, bhsparse_hip.hip) and its own kernels, bins and fill
// dispatch; the plumbing around them is here once: the workspace's set-up, the round trip of its control words, its two
// events, the kernel records' reset and read-out, the frame of a call that stands alone (side_open, side_start, side_close),
// the row pointer from a family's counts, the aliasing check of an entry point (side_aliased) and the guarded entry of the
// C-ABI.  For the graph and solver families, whose control blocks all begin with bhs_aggregate.hip.h's words: the lanes a row
// gets and their dispatch (side_lanes, with_lanes), the loop of rounds that decide until no vertex is left (side_rounds)
// and the loop of batched passes to a fixed point (side_passes, side_passes_within).

int wait_stream(bhs_handle* h);          // (bhs_host_pipeline.inc.h)

// A call starts: launches go to the handle's stream, the events and the pinned mirror exist from the first call on, the
// buffers hold ctlInts control words, queueBytes of per-bin queues and cntInts counts with the tile words of their scan
// (zeroed where newly allocated: see ensure).  0 for the queues or the counts: the family has none.
int side_prepare(bhs_handle* h, SideWs& ws, int ctlInts, size_t queueBytes, size_t cntInts)
{
    h->ls = h->stream;
    if (!ws.ev[0]) {
        BHS_HIP(hipEventCreate(&ws.ev[0]));
        BHS_HIP(hipEventCreate(&ws.ev[1]));
    }
    if (!ws.host) BHS_HIP(hipHostMalloc((void**)&ws.host, sizeof(int) * (size_t)ctlInts, hipHostMallocDefault));
    BHS_TRY(ensure(h, ws.ctl, sizeof(int) * (size_t)ctlInts));
    if (queueBytes) BHS_TRY(ensure(h, ws.queue, queueBytes));
    if (cntInts) {
        BHS_TRY(ensure(h, ws.cnt, sizeof(int) * cntInts));
        BHS_TRY(ensure(h, ws.tiles, sizeof(unsigned long long) * std::max<size_t>((cntInts - 1 + kScan1Tile - 1) / kScan1Tile, 1), true));
    }
    return BHS_SUCCESS;
}

// the first `ints` control words to the pinned mirror: a round trip of the call
int side_read_ctl(bhs_handle* h, SideWs& ws, int ints)
{
    BHS_HIP(hipMemcpyAsync(ws.host, ws.ctl.p, sizeof(int) * (size_t)ints, hipMemcpyDeviceToHost, h->stream));
    return wait_stream(h);
}

// the span a call reports as ms_out: from side_begin to side_end on the handle's stream
int side_begin(bhs_handle* h, SideWs& ws)
{
    BHS_HIP(hipEventRecord(ws.ev[0], h->stream));
    return BHS_SUCCESS;
}

int side_end(bhs_handle* h, SideWs& ws)
{
    BHS_HIP(hipEventRecord(ws.ev[1], h->stream));
    return BHS_SUCCESS;
}

int side_elapsed(bhs_handle* h, SideWs& ws, double* ms_out)
{
    if (ms_out) {
        float ms = 0;
        BHS_HIP(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        *ms_out = ms;
    }
    return BHS_SUCCESS;
}

// the kernel records of the last call make way for this one's (not where the call follows a multiply whose records stay)
void side_reset_stats(bhs_handle* h)
{
    h->evUsed = 0;
    for (auto& s : h->stats) { s.launches = 0; s.ms = 0; s.rows = s.products = s.nnz_out = s.nnzA_rows = 0; }
}

// the records' times from the event pairs evFirst onwards (those before it are a multiply's, read already)
int side_collect(bhs_handle* h, size_t evFirst)
{
    for (size_t i = evFirst; i < h->evUsed; ++i) {
        float ms = 0;
        BHS_HIP(hipEventElapsedTime(&ms, h->evPool[i].a, h->evPool[i].b));
        h->stats[h->evPool[i].stat].ms += ms;
    }
    return BHS_SUCCESS;
}

// The frame of a call that stands alone (none that follows a multiply and keeps its records), in three steps.  It opens:
// the workspace as side_prepare has it, its control block zeroed.  What else must be in place ahead of the span -- a control
// word at another identity, a buffer of the family's own -- goes between side_open and side_start.
int side_open(bhs_handle* h, SideWs& ws, int ctlInts, size_t queueBytes, size_t cntInts)
{
    BHS_TRY(side_prepare(h, ws, ctlInts, queueBytes, cntInts));
    BHS_HIP(hipMemsetAsync(ws.ctl.p, 0, sizeof(int) * (size_t)ctlInts, h->stream));
    return BHS_SUCCESS;
}

// the span starts: the last call's kernel records make way
int side_start(bhs_handle* h, SideWs& ws)
{
    side_reset_stats(h);
    return side_begin(h, ws);
}

// It closes behind side_end and the call's last round trip, which stay where the run function is read (a family's head
// comment counts its round trips, and the tests count them there): ms_out and the records' times.
int side_close(bhs_handle* h, SideWs& ws, double* ms_out)
{
    BHS_TRY(side_elapsed(h, ws, ms_out));
    return side_collect(h, 0);
}

// what an entry point answers where there is nothing to do and nothing is launched: no count, no round, no time
int side_nothing(int* count_out, int* rounds_out, double* ms_out)
{
    if (count_out) *count_out = 0;
    if (rounds_out) *rounds_out = 0;
    if (ms_out) *ms_out = 0.0;
    return BHS_SUCCESS;
}

// The tag of the next k_scan_onepass over `tiles`: the kernel takes a tile word for published where its 18-bit tag is this
// scan's, so a tag is not handed out twice while a word that carries it may still lie there -- every 2^18 scans the words of
// 2^18 scans ago could match: on the wrap the words are cleared (on the handle's stream, ahead of the scan) and the count
// starts again at 1, never at 0, the tag of a cleared word.
int scan_next_epoch(bhs_handle* h, unsigned& epoch, void* tiles, int nTiles)
{
    epoch = (epoch + 1) & 0x3FFFFu;
    if (epoch == 0) {
        BHS_HIP(hipMemsetAsync(tiles, 0, sizeof(unsigned long long) * (size_t)std::max(nTiles, 1), h->stream));
        epoch = 1;
    }
    return BHS_SUCCESS;
}

// where in a family's control block the scan keeps its words
struct SideScanWords {
    int ticket, total, bins, maxCnt;
};

// The row pointer from the `rows` counts in ws.cnt: the library's one-pass scan in place (tile words and epoch of the
// workspace's own, kernel record `name`), then a copy to where the row pointer is wanted.  The scan reads a row pointer of
// rows + 1 ints for its bins; without bins any such array will do: anyRowPtr.
int side_scan(bhs_handle* h, SideWs& ws, const char* name, const SideScanWords& w, int rows, const int* anyRowPtr, int* d_rowPtr)
{
    int* ctl = (int*)ws.ctl.p;
    int* cnt = (int*)ws.cnt.p;
    const int nTiles = (rows + kScan1Tile - 1) / kScan1Tile;
    if (nTiles == 0) {
        BHS_HIP(hipMemsetAsync(cnt, 0, sizeof(int), h->stream));
    } else {
        BHS_TRY(scan_next_epoch(h, ws.epoch, ws.tiles.p, nTiles));
        BinSpec none;                                                // (no bins: the scan's histogram stays empty)
        memset(&none, 0, sizeof(none));
        BHS_TRY(timed(h, name, rows, [&] {
            hipLaunchKernelGGL(k_scan_onepass, dim3((unsigned)nTiles), dim3(kScan1Block), 0, h->stream, rows, cnt, anyRowPtr,
                               (unsigned long long*)ws.tiles.p, ws.epoch, ctl + w.ticket, (long long*)(ctl + w.total), ctl + w.bins,
                               none, ctl + w.maxCnt, (const int*)nullptr);
            return 1;
        }));
    }
    BHS_HIP(hipMemcpyAsync(d_rowPtr, cnt, sizeof(int) * ((size_t)rows + 1), hipMemcpyDeviceToDevice, h->stream));
    return BHS_SUCCESS;
}

// do [a, a + na) and [b, b + nb) share a byte (a null or an empty range shares none)
bool rd_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// an array of a call, as its entry point sees it
struct Span {
    const void* p;
    size_t bytes;
};

// The aliasing check of an entry point: does an output overlap an input or another output.  An alias that a call permits
// (x == b of the triangular solve) is taken out of `ins` at the call site, where it can be seen.
bool side_aliased(std::initializer_list<Span> outs, std::initializer_list<Span> ins)
{
    for (const Span* o = outs.begin(); o != outs.end(); ++o) {
        for (const Span& i : ins)
            if (rd_overlap(o->p, o->bytes, i.p, i.bytes)) return true;
        for (const Span* p = o + 1; p != outs.end(); ++p)
            if (rd_overlap(o->p, o->bytes, p->p, p->bytes)) return true;
    }
    return false;
}

// ---- the graph and solver families (control words of bhs_aggregate.hip.h) ----------------------------------------------

// where their control blocks keep the scan's words
constexpr SideScanWords kAgScan = {AG_TICKET, AG_TOTAL, AG_BINS, AG_MAXCNT};

// lanes per row from a pattern's mean row length: 1, 4, 16 or 64
int side_lanes(long long n, long long nnz)
{
    const double mean = n > 0 ? (double)nnz / n : 0.0;
    return mean <= 4.0 ? 1 : mean <= 16.0 ? 4 : mean <= 64.0 ? 16 : 64;
}

// f(std::integral_constant<int, L>{}) for the L of side_lanes: a round function's result, or a kernel's pointer
template <typename F>
auto with_lanes(int L, F&& f)
{
    return L == 1 ? f(std::integral_constant<int, 1>{}) : L == 4 ? f(std::integral_constant<int, 4>{})
         : L == 16 ? f(std::integral_constant<int, 16>{}) : f(std::integral_constant<int, 64>{});
}

// The rounds that decide until no vertex of n is left (the aggregation, the colouring, the C/F splitting): launch(round,
// left) enqueues round 1, 2, ..'s kernels over the `left` vertices still undecided and returns a status; the loop clears the
// count ahead of it and makes the round's ONE round trip, of ctlInts control words, which stay in ws.host.  It ends when the
// count is zero, with BHS_ERR_INVALID_ARG when the error word is set, and with BHS_ERR_INTERNAL when a round decides nothing
// or after n + 1 rounds.  *rounds_out: the rounds whose words were read.
template <typename F>
int side_rounds(bhs_handle* h, SideWs& ws, long long n, int ctlInts, int* rounds_out, F&& launch)
{
    int* ctl = (int*)ws.ctl.p;
    long long left = n;
    for (long long round = 1;; ++round) {
        if (round > n + 1) return BHS_ERR_INTERNAL;
        BHS_HIP(hipMemsetAsync(ctl + AG_UNDEC, 0, sizeof(rd_u64), h->stream));
        BHS_TRY(launch(round, left));
        BHS_TRY(side_read_ctl(h, ws, ctlInts));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        long long now = 0;
        memcpy(&now, ws.host + AG_UNDEC, sizeof(now));
        *rounds_out = (int)round;
        if (now == 0) return BHS_SUCCESS;
        if (now >= left) return BHS_ERR_INTERNAL;                     // (the undecided vertex of greatest key is always decided)
        left = now;
    }
}

// The passes to a fixed point (the level sets, the components): `batch` passes of launch() a round trip of ctlInts control
// words, the clearInts words from AG_UNDEC on cleared ahead of the batch's last pass, so that they are that pass's alone.  It
// ends after a batch whose last pass counted nothing, and with BHS_ERR_INTERNAL when more than `bound` + 1 passes would be
// needed.  *passes_out: the passes launched.
template <typename F>
int side_passes_within(bhs_handle* h, SideWs& ws, long long bound, int batch, int clearInts, int ctlInts, int* passes_out, F&& launch)
{
    int* ctl = (int*)ws.ctl.p;
    long long passes = 0;
    for (;;) {
        if (passes > bound) return BHS_ERR_INTERNAL;
        for (int p = 0; p < batch; ++p) {
            if (p == batch - 1) BHS_HIP(hipMemsetAsync(ctl + AG_UNDEC, 0, sizeof(int) * (size_t)clearInts, h->stream));
            BHS_TRY(launch());
        }
        passes += batch;
        BHS_TRY(side_read_ctl(h, ws, ctlInts));
        if (ws.host[RD_ERR]) return BHS_ERR_INVALID_ARG;
        long long count = 0;
        memcpy(&count, ws.host + AG_UNDEC, sizeof(count));
        *passes_out = (int)std::min<long long>(passes, 0x7fffffff);
        if (count == 0) return BHS_SUCCESS;
    }
}

// ... where a pass changes one of n things at least: more than n + 1 passes are never needed (n passes change something, one
// more finds nothing)
template <typename F>
int side_passes(bhs_handle* h, SideWs& ws, long long n, int batch, int clearInts, int ctlInts, int* passes_out, F&& launch)
{
    return side_passes_within(h, ws, n, batch, clearInts, ctlInts, passes_out, launch);
}

// after a failed call: nothing of it stays queued (the pipeline's own state is not touched)
void settle(bhs_handle* h)
{
    (void)hipStreamSynchronize(h->stream);
    (void)hipGetLastError();
}

// What an entry point of the C-ABI does once it has accepted its arguments, through here: `body` on the handle's device, and
// whatever makes it fail -- a run's result, or a BHS_HIP / BHS_TRY of a staging copy written in the body itself -- leaves
// nothing queued on the handle's stream.
template <typename F>
int guarded(bhs_handle* h, F&& body)
{
    BHS_HIP(hipSetDevice(h->device));
    const int rc = body();
    if (rc) settle(h);
    return rc;
}
