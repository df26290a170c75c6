// bhs_host_side.inc.h -- what the operations beside the multiply pipeline share on the host: the masked and the semiring
// multiply, the sparse add, the entry selection, the transpose, the extraction, the reductions and the scaling
// (A part of bhsparse_hip.hip's translation unit: included there inside its unnamed namespace, ahead of the pipeline, whose
// scan takes its epochs from here too.)
//
// Every family keeps a workspace of its own on the handle (SideWs, bhsparse_hip.hip) and its own kernels, bins and fill
// dispatch; the plumbing around them is here once: the workspace's set-up, the round trip of its control words, its two
// events, the kernel records' reset and read-out, the row pointer from a family's counts, and the guarded entry of the C-ABI.

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

// do [a, a + na) and [b, b + nb) share a byte (an output array against an input: the reductions, the scaling, CSR x dense)
bool rd_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
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
