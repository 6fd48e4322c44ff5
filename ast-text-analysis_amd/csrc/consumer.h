// consumer.h -- the host frame of the handle's consumers: the cosine term index, the keyphrase graph, the synonyms, the
// ranking, the similarity, the text-to-text relatedness, the text-to-text cosine, the clusters, the extracted phrases,
// the characteristic terms, the shingle overlap and the shared passages.
// A consumer is a struct of device buffers and results that the handle owns beside its arena, made by its first call.  The frame has
// the state and its lifetime, the timer, the front of every entry point (consumer_begin, consumer_built, the two halves
// of a *_build_resident / *_build_host pair), the table a source names (resolve_table), the M x M matrix of the consumers
// that produce one (MatrixConsumer) and the count-scan-fill of a list of unknown length.  Nothing in here knows one
// consumer from another but OFFERED, the table of sources behind resolve_table and consumer_resident_square ("The
// consumer frame").
#pragma once
#include "handle.h"
#include "scan.h"

// ---- a score table on the device ------------------------------------------------------------------------------------------
struct TableRef {               // K x D doubles on the handle's device, ordered behind everything queued on its stream
    const double *p = nullptr;  // (nullptr: no table)
    u32 K = 0, D = 0;
    bool directed = false;      // a square matrix whose [a][b] and [b][a] are two values (the clusters take no such)
};

// ---- state, lifetime, timing ----------------------------------------------------------------------------------------------
struct Consumer {
    bool valid = false;                     // the last build's result can be fetched
    float ms = -1.f;                        // device time of the last call that succeeded; -1 from the start of a call until it has
    hipEvent_t ev0 = nullptr, ev1 = nullptr;    // (made by the first ConsumerTimer)
    std::vector<DevBuf *> bufs;             // every device allocation of the consumer (its constructor lists them)
    size_t keep_bytes = 0;                  // east_hip_reset releases the buffers larger than this

    Consumer() = default;
    Consumer(const Consumer &) = delete;    // (bufs points into the object)
    virtual void clear() = 0;               // the consumer's own fields, back to "nothing built"
    virtual TableRef offers() const { return TableRef(); }      // the score table other consumers may read where it lies
    void withdraw()                         // the result is no longer there to fetch; the buffers stay
    {
        valid = false;
        ms = -1.f;
    }
    void reset()
    {
        withdraw();
        clear();
        for (DevBuf *b : bufs)
            if (b->cap > keep_bytes) b->release();
    }
    virtual ~Consumer()
    {
        for (DevBuf *b : bufs) b->release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// T::SLOT names T's place in the handle.  consumer_peek: nullptr before the consumer's first call; consumer_state makes it.
template <class T> static T *consumer_peek(const east_hip_index *h) { return static_cast<T *>(h->consumers[T::SLOT]); }
template <class T> static T &consumer_state(east_hip_index *h)
{
    if (!h->consumers[T::SLOT]) h->consumers[T::SLOT] = new T();
    return *consumer_peek<T>(h);
}
// The front of a build: T's state, its last result withdrawn.
template <class T> static T &consumer_begin(east_hip_index *h)
{
    T &g = consumer_state<T>(h);
    g.withdraw();
    return g;
}
// The front of a fetch: T's state with a result to fetch, on the handle's device; none: the message of EAST_HIP_ERR_NOT_BUILT.
template <class T> static T &consumer_built(east_hip_index *h, const char *none)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    T *g = consumer_peek<T>(h);
    if (!g || !g->valid) east_throw(EAST_HIP_ERR_NOT_BUILT, none);
    use_device(h);
    return *g;
}
template <class T> static double consumer_ms(const east_hip_index *h) { return h && h->consumers[T::SLOT] ? (double)h->consumers[T::SLOT]->ms : -1.0; }

// Brackets a call's launches on the handle's stream: ev0 now; finish() records ev1, waits for the stream and stores the time.
// stop() records ev1 early, for a call that queues behind its launches what it does not count (the copy of a table to the host).
struct ConsumerTimer {
    east_hip_index *h;
    Consumer &c;
    bool stopped = false;
    ConsumerTimer(east_hip_index *h_, Consumer &c_) : h(h_), c(c_)
    {
        if (!c.ev1) {
            if (!c.ev0) HIP_CHECK(hipEventCreate(&c.ev0));
            HIP_CHECK(hipEventCreate(&c.ev1));
        }
        HIP_CHECK(hipEventRecord(c.ev0, h->stream));
    }
    void stop()
    {
        HIP_CHECK(hipEventRecord(c.ev1, h->stream));
        stopped = true;
    }
    void finish()
    {
        if (!stopped) stop();
        HIP_CHECK(hipStreamSynchronize(h->stream));
        HIP_CHECK(hipEventElapsedTime(&c.ms, c.ev0, c.ev1));
    }
};

// ---- a host table's copy --------------------------------------------------------------------------------------------------
// Every consumer that takes a host table keeps a copy of its OWN (include/east_hip.h promises that they are separate).
struct UploadedTable {
    DevBuf buf;
    u32 K = 0, D = 0;                       // K x D while the copy is whole, 0 x 0 while there is none or it is being replaced
    TableRef ref() const
    {
        TableRef t;
        if (K) { t.p = (const double *)buf.p; t.K = K; t.D = D; }
        return t;
    }
    void withdraw() { K = D = 0; }
    TableRef upload(east_hip_index *h, const double *table, u32 n_keyphrases, u32 n_docs, const char *what)
    {
        withdraw();
        const size_t bytes = (size_t)n_keyphrases * (size_t)n_docs * 8;
        buf.ensure(bytes, what, h->stream);
        HIP_CHECK(hipMemcpyAsync(buf.p, table, bytes, hipMemcpyHostToDevice, h->stream));
        HIP_CHECK(hipStreamSynchronize(h->stream));
        K = n_keyphrases;
        D = n_docs;
        return ref();
    }
};

// ---- which table a *_build_resident call reads ----------------------------------------------------------------------------
// What a consumer offers(), a row a source.  matrix: a square matrix of members (the similarity's, the relatedness', the
// text-to-text cosine's, the shingle overlap's); directed: what a consumer of symmetric matrices says of its directed form.
static const struct Offered { int32_t source; int slot; bool matrix; const char *missing, *directed; } OFFERED[] = {
    {EAST_HIP_GRAPH_SOURCE_COSINE, east_hip_index::SLOT_COS, false, ": no cosine score table is resident (score the keyphrases first)", nullptr},
    {EAST_HIP_GRAPH_SOURCE_SIMILARITY, east_hip_index::SLOT_SIM, true, ": no similarity matrix has been built on this handle", nullptr},
    {EAST_HIP_GRAPH_SOURCE_RELATED, east_hip_index::SLOT_REL, true, ": no relatedness matrix has been built on this handle",
     ": the relatedness matrix is directed (build it with EAST_HIP_RELATED_SYMMETRIC)"},
    {EAST_HIP_GRAPH_SOURCE_COSINE_TEXTS, east_hip_index::SLOT_COSTEXT, true, ": no text similarity matrix has been built on this handle", nullptr},
    {EAST_HIP_GRAPH_SOURCE_OVERLAP, east_hip_index::SLOT_OVL, true, ": no overlap matrix has been built on this handle",
     ": the overlap matrix is directed (build it with EAST_HIP_OVERLAP_SYMMETRIC)"},
};

// who: the consumer's name in front of its messages; own: the caller's uploaded copy (nullptr before its first call);
// matrices_ok: the square matrices other consumers built are sources too (the ranking and the clusters).
static TableRef resolve_table(const east_hip_index *h, int32_t source, const UploadedTable *own, const char *who, bool matrices_ok = false)
{
    TableRef t;
    const char *missing = nullptr;
    if (source == EAST_HIP_GRAPH_SOURCE_AST) {
        if (h->built && h->table_scored) { t.p = h->kp.table; t.K = h->kp.n_kp; t.D = h->n_docs; }
        missing = ": no score table is resident (score the keyphrases first)";
    } else if (source == EAST_HIP_GRAPH_SOURCE_UPLOADED) {
        if (own) t = own->ref();
        missing = ": no host table has been uploaded to this handle";
    }
    for (const Offered &o : OFFERED)
        if (o.source == source && (matrices_ok || !o.matrix)) {
            if (h->consumers[o.slot]) t = h->consumers[o.slot]->offers();
            missing = o.missing;
        }
    if (!missing) east_throw(EAST_HIP_ERR_INVALID, std::string(who) + ": unknown table source");
    if (!t.p) east_throw(EAST_HIP_ERR_NOT_BUILT, std::string(who) + missing);
    return t;
}

// ---- the two halves of a *_build_resident / *_build_host pair ---------------------------------------------------------------
// T has an UploadedTable `table`.  The resident half: the table the source names, on the handle's device.
template <class T> static TableRef consumer_resident(east_hip_index *h, int32_t source, const char *who, bool matrices_ok = false)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    use_device(h);
    const T *g = consumer_peek<T>(h);
    return resolve_table(h, source, g ? &g->table : nullptr, who, matrices_ok);
}

// The resident half of a consumer that takes only symmetric square matrices of members (the clusters): any other source is
// refused before anything is resolved, a directed matrix in its row's own words.
template <class T> static TableRef consumer_resident_square(east_hip_index *h, int32_t source, const char *who)
{
    const Offered *row = nullptr;
    for (const Offered &o : OFFERED)
        if (o.source == source && o.matrix) row = &o;
    if (!row && source != EAST_HIP_GRAPH_SOURCE_UPLOADED)
        east_throw(EAST_HIP_ERR_INVALID, std::string(who) + ": the source is not a square matrix of members");
    const TableRef t = consumer_resident<T>(h, source, who, true);
    if (t.directed && !(row && row->directed)) east_throw(EAST_HIP_ERR_INTERNAL, std::string(who) + ": OFFERED[] has no words for this directed matrix");
    if (t.directed) east_throw(EAST_HIP_ERR_INVALID, std::string(who) + row->directed);
    if (t.K != t.D) east_throw(EAST_HIP_ERR_INTERNAL, std::string(who) + ": the source matrix is not square");
    return t;
}

// The host half: the host table's copy on the device, T's last result withdrawn.  empty: the message for no table; check()
// throws for what else can be refused BEFORE the upload (a call refused there leaves the uploaded table alone); what the
// caller checks on the TableRef that comes back is checked AFTER it (the new table is the uploaded one by then).
template <class T, class Check>
static TableRef consumer_upload(east_hip_index *h, const double *table, int32_t n_keyphrases, int32_t n_docs, const char *empty,
                                const char *what, Check check)
{
    if (!h) east_throw(EAST_HIP_ERR_INVALID, "null handle");
    if (!table || n_keyphrases < 1 || n_docs < 1) east_throw(EAST_HIP_ERR_INVALID, empty);
    check();
    use_device(h);
    return consumer_begin<T>(h).table.upload(h, table, (u32)n_keyphrases, (u32)n_docs, what);
}

// ---- an M x M matrix of members ------------------------------------------------------------------------------------------
// The similarity, the relatedness and the text-to-text cosine: a matrix the ranking and the clusters read where it lies, a
// double a member (the similarity's squared norms, the others' diagonal before the NaN) and, for two of them, a count a
// member (the relatedness' scored strings, the text cosine's postings).
#define MATRIX_MAX_M (1u << 20)            // (8 TiB of matrix: more than any device holds; 2^14 tiles a grid dimension)

struct MatrixConsumer : Consumer {
    u32 M = 0;
    DevBuf out;                             // matrix, per_member, count
    double *matrix = nullptr, *per_member = nullptr;
    int32_t *count = nullptr;               // (nullptr: the consumer has none)
    MatrixConsumer() { bufs = {&out}; }     // (a derived state adds its own)
    void clear() override
    {
        M = 0;
        matrix = per_member = nullptr;
        count = nullptr;
    }
    TableRef offers() const override        // (the ranking and the clusters read the matrix where it lies)
    {
        TableRef t;
        if (valid) { t.p = matrix; t.K = t.D = M; }
        return t;
    }
};

// EAST_HIP_ERR_OOM in the one wording; of: the size in the consumer's own nouns ("12 texts")
[[noreturn]] static void consumer_oom(const char *who, const char *what, const std::string &of, double bytes)
{
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: %s of %s needs %.0f bytes, which the device does not have", who, what, of.c_str(), bytes);
    east_throw(EAST_HIP_ERR_OOM, msg);
}

// Room for M members in g.out, carved; the limit is tested before anything is allocated.
static void matrix_reserve(east_hip_index *h, MatrixConsumer &g, u32 M, bool with_count, const char *who, const std::string &of)
{
    const size_t bytes = align256((size_t)M * M * 8) + align256((size_t)M * 8) + (with_count ? align256((size_t)M * 4) : 0) + 256;
    if (M > MATRIX_MAX_M || !g.out.try_ensure(bytes, h->stream)) consumer_oom(who, "the matrix", of, (double)M * (double)M * 8.0);
    Arena a = g.out.arena();
    g.matrix = a.alloc<double>((size_t)M * M);
    g.per_member = a.alloc<double>(M);
    g.count = with_count ? a.alloc<int32_t>(M) : nullptr;
    g.M = M;
}

// what the caller has room for; g comes from consumer_built
static void matrix_fetch(east_hip_index *h, const MatrixConsumer &g, double *matrix, double *per_member, int32_t *count)
{
    if (matrix) HIP_CHECK(hipMemcpyAsync(matrix, g.matrix, (size_t)g.M * g.M * 8, hipMemcpyDeviceToHost, h->stream));
    if (per_member) HIP_CHECK(hipMemcpyAsync(per_member, g.per_member, (size_t)g.M * 8, hipMemcpyDeviceToHost, h->stream));
    if (count) HIP_CHECK(hipMemcpyAsync(count, g.count, (size_t)g.M * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
}

// ---- count, scan, fill ----------------------------------------------------------------------------------------------------
// A list of unknown length written without an atomic: a first pass counts per (row, target block), the exclusive scan of the
// counts in that order gives every block's offset inside its row (modulo 2^32: differences inside a row are exact), the
// kernel below the 64-bit number of entries in front of every row, and a second pass writes every entry to its slot.

// row_base[s] = edges of the sources in front of s, in 64 bits; row_base[M] = all edges.  One workgroup: M values.
__global__ __launch_bounds__(BLOCK) void graph_row_base_kernel(const u32 *__restrict__ cnt_ex, u32 M, u32 TB, u64 *__restrict__ row_base)
{
    __shared__ u32 lds4[WAVES_PER_BLOCK];
    u64 carry = 0;
    for (u32 b = 0; b < M; b += BLOCK) {
        const u32 s = b + threadIdx.x;
        const u32 x = s < M ? cnt_ex[(size_t)(s + 1u) * TB] - cnt_ex[(size_t)s * TB] : 0u;      // (at most M - 1 each: 256 of them fit 32 bits)
        u32 total = 0;
        const u32 ex = block_exclusive_sum(x, lds4, total);
        if (s < M) row_base[s] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) row_base[M] = carry;
}

struct EmitCounts {
    u32 rows, TB, n;            // n = rows * TB counts + the sentinel the scan leaves the total in
    size_t bytes;               // what the counts, the row bases and the scan's scratch take of the caller's arena
};

// too_many: the message of EAST_HIP_ERR_INVALID when the counts do not fit one scan (a printf format: %u = rows)
static EmitCounts emit_counts(u32 rows, u32 TB, const char *too_many)
{
    const u64 n = (u64)rows * TB + 1;
    if (n >= (u64)0xFFFFFFF0u) {
        char msg[160];
        snprintf(msg, sizeof(msg), too_many, rows);
        east_throw(EAST_HIP_ERR_INVALID, msg);
    }
    return EmitCounts{rows, TB, (u32)n, n * 4 + ((size_t)rows + 1) * 8 + ((size_t)ceil_div_u32(n, SCAN_TILE) + 1) * 8 + 16 * 256};
}

// ctx.arena: the caller's, with e.bytes to spare.  count(cnt) launches the counting pass; zero_all: it leaves counts unwritten,
// which are to read 0.  size(total) makes room for a total > 0; fill(cnt, row_base) launches the filling pass.  One
// synchronisation: the read-back of the total, which is returned.
template <class Count, class Size, class Fill>
static u64 emit_count_scan_fill(Ctx &ctx, const EmitCounts &e, bool zero_all, Count count, Size size, Fill fill)
{
    u32 *cnt = ctx.arena->alloc<u32>(e.n);
    u64 *row_base = ctx.arena->alloc<u64>((size_t)e.rows + 1);
    if (zero_all) HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)e.n * 4, ctx.stream));
    else HIP_CHECK(hipMemsetAsync(cnt + (e.n - 1u), 0, 4, ctx.stream));
    count(cnt);
    device_scan<ArrIn, false>(ctx, ArrIn{cnt}, e.n, cnt);
    LAUNCH(ctx, graph_row_base_kernel, 1, (const u32 *)cnt, e.rows, e.TB, row_base);
    u64 total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, row_base + e.rows, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_CHECK(hipStreamSynchronize(ctx.stream));
    if (total) {
        size(total);
        fill(cnt, (const u64 *)row_base);
    }
    return total;
}
