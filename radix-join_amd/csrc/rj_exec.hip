// rj_exec.hip — plan executor: the host logic of Contest::execute on MI355X.
//
// Replaces reference src/execute.cpp:266-324 (execute, execute_impl, execute_scan,
// execute_hash_join, hash_join_omp).  Shape: columnar + late materialisation.
//   * A node's result ("Rel") is a set of device columns: regular page images
//     addressed in place, dense arrays, or row-id columns standing for VARCHAR.
//   * A JoinNode radix-partitions (hashed key, carry) tuples of both children
//     with the same bit plan, joins co-partitions in LDS and emits up to three
//     streams: key, build carry, probe carry.  The carry is the single payload
//     column itself when a side needs only one (no gather afterwards), else the
//     row index into the child, gathered per output column.
//   * At the root the streams are written straight into Page images.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <set>
#include <tuple>

#include "rj_expr.hpp"
#include "rj_internal.hpp"
#include "rj_radix.hpp"
#include "rj_xplan.hpp"

namespace rj {

// What the plan walks know about a node kind: Exec::node, ShardedExec, first_unshardable and the
// uploader's scan_order (rj_table.hip).  A new kind gets its line here, its driver in Exec and, if it has
// one child, its case in Exec::node's switch (without one the walk reports "bad node kind"); a kind with
// two children that is not a join is handed to its driver in front of join_kind().
const NodeKind* node_kind(int kind) {
    static const NodeKind kinds[] = {
        {RJ_NODE_SCAN, "a scan", "RJ_NODE_SCAN", 0, true},
        {RJ_NODE_JOIN, "a join", "RJ_NODE_JOIN", 2, true},
        {RJ_NODE_SEMI, "a semi join", "RJ_NODE_SEMI", 2, false},
        {RJ_NODE_ANTI, "an anti join", "RJ_NODE_ANTI", 2, false},
        {RJ_NODE_OUTER, "an outer join", "RJ_NODE_OUTER", 2, false},
        {RJ_NODE_FULL, "a full outer join", "RJ_NODE_FULL", 2, false},
        {RJ_NODE_AGG, "an aggregation", "RJ_NODE_AGG", 1, false},
        {RJ_NODE_SELECT, "a selection", "RJ_NODE_SELECT", 1, false},
        {RJ_NODE_SORT, "a sort", "RJ_NODE_SORT", 1, false},
        {RJ_NODE_GROUP, "a grouping", "RJ_NODE_GROUP", 1, false},
        {RJ_NODE_WINDOW, "a window", "RJ_NODE_WINDOW", 1, false},
        {RJ_NODE_MAP, "a map", "RJ_NODE_MAP", 1, false},
        {RJ_NODE_SETOP, "a set operation", "RJ_NODE_SETOP", 2, false},
    };
    for (const NodeKind& k : kinds)
        if (k.kind == kind) return &k;
    return nullptr;
}

namespace {

// a buffer's memory, or nullptr where there is no buffer
template <class T>
T* ptr(const BufP& b) {
    return b ? b->as<T>() : nullptr;
}

struct DCol {
    int32_t        type = RJ_INT32;  // declared DataType
    int32_t        kind = COL_NONE;
    int32_t        width = 4;  // bytes per value on device (VARCHAR: 4 = row id)
    const uint8_t* ptr = nullptr;
    const uint8_t* valid = nullptr;
    BufP           hold, hold_valid;
    int            vc_table = -1, vc_col = -1;  // VARCHAR provenance (base table, column)
    const TableColumn* tcol = nullptr;          // scan passthrough
    ColRef ref() const { return ColRef{ptr, valid, kind, width}; }
};

struct Rel {
    uint64_t          n = 0;
    std::vector<DCol> cols;
};

struct JoinSpec {
    bool                  build_left = true;
    uint64_t              left_attr = 0, right_attr = 0;
    std::vector<uint64_t> out_idx;
    std::vector<int32_t>  out_type;
    bool                  prehashed = false;
    int                   forced_bits = 0;
    uint32_t              top_bits_taken = 0;  // high hash bits that are constant in this input
};

JoinSpec join_spec(const rj_node& n, int forced_bits) {
    JoinSpec js;
    js.build_left = n.build_left != 0;
    js.left_attr = n.left_attr;
    js.right_attr = n.right_attr;
    js.out_idx.assign(n.out_idx, n.out_idx + n.n_out);
    js.out_type.assign(n.out_type, n.out_type + n.n_out);
    js.forced_bits = forced_bits;
    return js;
}

// What tells the five join node kinds apart outside their own functions.  The build side of
// SEMI / ANTI is the filter side (it carries nothing); an optional side's columns come out NULL in
// the rows that have no partner on that side.
struct JoinKind {
    int         node;             // RJ_NODE_*
    const char* name;             // in messages and diagnostics
    bool        emits_unmatched;  // probe rows without a partner come out too
    bool        build_optional, probe_optional;
    int         attempts;         // of the probe: 1 = the first streams hold any result, 2 = rerun at the exact size
};
const JoinKind& join_kind(int node) {
    static const JoinKind kinds[] = {
        {RJ_NODE_JOIN, "join", false, false, false, 2},
        {RJ_NODE_SEMI, "semi join", false, false, false, 1},
        {RJ_NODE_ANTI, "anti join", true, false, false, 1},
        {RJ_NODE_OUTER, "outer join", true, true, false, 2},
        {RJ_NODE_FULL, "full outer join", true, true, true, 2},
    };
    for (const JoinKind& k : kinds)
        if (k.node == node) return k;
    throw_fmt(RJ_ERR_ARG, "bad node kind");
}

uint32_t ceil_log2(uint64_t v) {
    uint32_t b = 0;
    while ((uint64_t(1) << b) < v) ++b;
    return b;
}

class Exec {
   public:
    Exec(Context* c, const rj_plan* p, Table* const* t, uint64_t nt, int fl)
        : ctx(c), plan(p), tables(t), n_tables(nt), flags(fl), L(c->launch()) {}
    void set_fetch(TableFetch* f) { fetch = f; }

    Result* run() {
        if (!plan || plan->root >= plan->n_nodes) throw_fmt(RJ_ERR_ARG, "bad plan root");
        std::unique_ptr<Result> res(new rj_result());
        res->ctx = ctx;
        const rj_node& root = plan->nodes[plan->root];
        if (root.kind == RJ_NODE_SCAN) {
            root_scan(root, *res);
        } else {
            (void)node(plan->root, res.get(), 0);
        }
        ctx->sync();
        return res.release();
    }

    // rj_join_tuples: same join core over caller-provided dense tuples
    Result* run_tuples(const rj_tuples* b, const rj_tuples* p, uint32_t skip_rank_bits) {
        std::unique_ptr<Result> res(new rj_result());
        res->ctx = ctx;
        auto mk = [](const rj_tuples* t) {
            Rel r;
            r.n = t->n;
            DCol k = dense_col(RJ_INT32, BufP());  // (the caller's arrays: nothing to hold)
            k.ptr = static_cast<const uint8_t*>(t->key);
            DCol c = k;
            c.ptr = static_cast<const uint8_t*>(t->carry);
            r.cols = {k, c};
            return r;
        };
        if (b->n > 0xfffffff0ull || p->n > 0xfffffff0ull)
            throw_fmt(RJ_ERR_UNSUPPORTED, "more than 2^32 tuples");
        if (b->hashed != p->hashed) throw_fmt(RJ_ERR_ARG, "build/probe disagree on `hashed`");
        Rel      lb = mk(b), rp = mk(p);
        JoinSpec js;
        js.build_left = true;
        js.out_idx = {0, 1, 3};
        js.out_type = {RJ_INT32, RJ_INT32, RJ_INT32};
        js.prehashed = b->hashed != 0;
        // the top hash bits stage A consumed are constant on this rank: the radix plan stays
        // below them (they would only produce empty partitions)
        if (skip_rank_bits > 16) throw_fmt(RJ_ERR_ARG, "skip_rank_bits > 16");
        js.top_bits_taken = js.prehashed ? skip_rank_bits : 0u;
        (void)join_core(lb, rp, js, res.get());
        ctx->sync();
        return res.release();
    }

    // rj_shard_partition: decode + hash + one pass over the TOP log2(n_ranks) hash bits
    void run_shard(const Table* t, uint64_t key_col, uint64_t carry_col, uint32_t n_ranks,
                   rj_tuples* out, uint64_t* counts) {
        if (n_ranks == 0 || (n_ranks & (n_ranks - 1)) || n_ranks > (1u << PT_MAXBITS))
            throw_fmt(RJ_ERR_UNSUPPORTED, "n_ranks must be a power of two <= %d", 1 << PT_MAXBITS);
        if (key_col >= t->cols.size() || carry_col >= t->cols.size())
            throw_fmt(RJ_ERR_ARG, "column out of range");
        DCol k = table_col(t, (int)key_col), c = table_col(t, (int)carry_col);
        if (k.type != RJ_INT32 || c.type != RJ_INT32)
            throw_fmt(RJ_ERR_UNSUPPORTED, "sharded path carries INT32 key + INT32 payload");
        if (c.valid) throw_fmt(RJ_ERR_UNSUPPORTED, "sharded path: payload column has NULLs");
        TupleSrc src{};
        src.key = k.ref();
        src.carry = c.ref();
        src.n_rows = (uint32_t)t->num_rows;
        src.carry_mode = CARRY_COLUMN;
        if (!out->key || !out->carry) throw_fmt(RJ_ERR_ARG, "rj_shard_partition: null output buffers");
        uint32_t rb = ceil_log2(n_ranks);
        Words    ext{};
        ext.w[0] = static_cast<uint32_t*>(out->key);
        ext.w[1] = static_cast<uint32_t*>(out->carry);
        PartitionRequest rq = PartitionRequest::columns(src, 1, 1, rb);
        rq.shift0 = rb ? 32 - rb : 31;
        rq.single_pass = true;
        rq.external = &ext;
        Parted P = partition(rq);
        std::vector<uint32_t> off(n_ranks + 1);
        read_back(off.data(), P.off->p, (n_ranks + 1) * 4);
        for (uint32_t r = 0; r < n_ranks; ++r) counts[r] = off[r + 1] - off[r];
        out->n = off[n_ranks];
        out->hashed = 1;
        out->reserved = 0;
    }

    // ---- state and building blocks (a ShardedExec drives one Exec per rank through them)
    Context*       ctx;
    const rj_plan* plan;
    Table* const*  tables;
    uint64_t       n_tables;
    int            flags;
    TableFetch*    fetch = nullptr;
    Launch         L;
    std::map<std::pair<const Table*, int>, DCol> decoded_;
    std::map<std::pair<int, int>, std::vector<uint64_t>> vc_dir_;  // VARCHAR page directories

    // ------------------------------------------------------------- columns
    // bytes per value on the device (VARCHAR: a row id)
    static int width_of(int32_t type) { return type == RJ_INT32 || type == RJ_VARCHAR ? 4 : 8; }
    // a dense column over existing arrays (either may be none: no rows, no NULLs)
    static DCol dense_col(int32_t type, const BufP& values, const BufP& valid = BufP()) {
        DCol d;
        d.type = type;
        d.kind = COL_DENSE;
        d.width = width_of(type);
        d.hold = values;
        d.ptr = ptr<uint8_t>(values);
        d.hold_valid = valid;
        d.valid = ptr<uint8_t>(valid);
        return d;
    }
    // ... of `src`'s type, with its VARCHAR provenance
    static DCol dense_like(const DCol& src, const BufP& values, const BufP& valid = BufP()) {
        DCol d = dense_col(src.type, values, valid);
        d.vc_table = src.vc_table;
        d.vc_col = src.vc_col;
        return d;
    }
    // ... over new arrays of `rows` values
    DCol new_col(int32_t type, uint64_t rows, bool nullable) {
        BufP values = ctx->buf(rows * width_of(type));
        return dense_col(type, values, nullable ? ctx->buf(rows) : BufP());
    }

    static void check_rows(const Rel& r) {
        if (r.n > 0xfffffff0ull) throw_fmt(RJ_ERR_UNSUPPORTED, "more than 2^32 rows in one relation");
    }

    // `bytes` from the device into `dst`, waited for (the stream drains before an exception travels on)
    void read_back(void* dst, const void* src, size_t bytes) { rj::read_back(ctx, dst, src, bytes); }

    // Where the columns of a one-child node's output go: below the root into the Rel its parent reads,
    // at the root into the Result as Page images.
    struct Sink {
        Exec*   E;
        Result* res;  // the root's result, or nullptr below the root
        Rel     out;
        std::map<uint64_t, DCol>         made;     // per id ...
        std::map<uint64_t, ResultColumn> encoded;  // ... and its pages at the root
        Sink(Exec* e, Result* root_res, uint64_t rows) : E(e), res(root_res) {
            out.n = rows;
            if (res) res->num_rows = rows;
        }
        // a column of its own
        void add(const DCol& d) {
            if (res)
                res->cols.push_back(E->col_to_result(d, out.n));
            else
                out.cols.push_back(d);
        }
        // a column that may be named several times: `make` runs, and the root encodes, once per id
        template <class Make>
        void add(uint64_t id, Make&& make) {
            if (!made.count(id)) made[id] = make();
            if (!res) {
                out.cols.push_back(made.at(id));
                return;
            }
            if (!encoded.count(id)) encoded[id] = E->col_to_result(made.at(id), out.n);
            res->cols.push_back(encoded.at(id));
        }
    };

    // ------------------------------------------------------------- scan side
    DCol table_col(const Table* t, int c) {
        const TableColumn& tc = t->cols[c];
        if (tc.skipped) throw_fmt(RJ_ERR_ARG, "column was not uploaded (not referenced by a scan)");
        DCol d = dense_col(tc.type, BufP());
        d.tcol = &tc;
        if (tc.type == RJ_VARCHAR) {
            d.kind = COL_IOTA;
            return d;
        }
        if (t->num_rows == 0) return d;  // nothing to address (an empty shard): no validity to carry either
        if (tc.regular) {
            d.kind = COL_PAGED;
            d.ptr = tc.dev_pages;
            return d;
        }
        auto key = std::make_pair(t, c);
        auto it = decoded_.find(key);
        if (it != decoded_.end()) return it->second;
        // K1: irregular pages (NULLs, short pages) -> dense values + validity
        uint64_t n = t->num_rows;
        d = new_col(tc.type, n, true);
        d.tcol = &tc;
        RJ_HIP(hipMemsetAsync(d.hold->p, 0, n * d.width, ctx->stream));
        RJ_HIP(hipMemsetAsync(d.hold_valid->p, 0, n, ctx->stream));
        if (tc.n_pages) {
            BufP row_base = ctx->buf((tc.n_pages + 1) * 4);
            launch_scan_bins(L, tc.page_rows->as<uint32_t>(), (uint32_t)tc.n_pages,
                             row_base->as<uint32_t>(), nullptr);
            launch_decode_pages(L, tc.dev_pages, (uint32_t)tc.n_pages, d.width,
                                row_base->as<uint32_t>(), n, d.hold->as<uint8_t>(),
                                d.hold_valid->as<uint8_t>());
        }
        decoded_[key] = d;
        return d;
    }

    const Table* table_of(const rj_node& n) {
        return table_by_id(n.base_table_id);
    }
    const Table* table_by_id(uint64_t id) {
        if (id >= n_tables) throw_fmt(RJ_ERR_ARG, "scan: bad base_table_id");
        return fetch ? fetch->get(id) : tables[id];
    }

    // execute_scan (reference src/execute.cpp:284-300): column selection, zero copy
    Rel scan(const rj_node& n) {
        const Table* t = table_of(n);
        Rel          r;
        r.n = t->num_rows;
        for (uint64_t k = 0; k < n.n_out; ++k) {
            uint64_t c = n.out_idx[k];
            if (c >= t->cols.size()) throw_fmt(RJ_ERR_ARG, "scan: output attr out of range");
            if (t->cols[c].type != n.out_type[k])
                throw_fmt(RJ_ERR_ARG, "scan: declared type differs from the column's type");
            DCol d = table_col(t, (int)c);
            if (d.type == RJ_VARCHAR) {
                d.vc_table = (int)n.base_table_id;
                d.vc_col = (int)c;
            }
            r.cols.push_back(d);
        }
        return r;
    }

    // A plan whose root is a Scan.  The result's pages have to add up to num_rows rows, which the
    // input's pages need not: they may cover fewer rows (the rest is NULL) or carry NULL rows past the
    // end (reference src/build_table.cpp:326-343 reads both).  So only a regular fixed-width column,
    // and a VARCHAR column whose pages hold exactly num_rows rows, hand their input pages out; any
    // other column is decoded and encoded again, as the reference does with every column.
    void root_scan(const rj_node& n, Result& res) {
        const Table* t = table_of(n);
        res.num_rows = t->num_rows;
        for (uint64_t k = 0; k < n.n_out; ++k) {
            uint64_t c = n.out_idx[k];
            if (c >= t->cols.size()) throw_fmt(RJ_ERR_ARG, "scan: output attr out of range");
            const TableColumn& tc = t->cols[c];
            if (tc.type != n.out_type[k])
                throw_fmt(RJ_ERR_ARG, "scan: declared type differs from the column's type");
            ResultColumn rc;
            rc.type = tc.type;
            if (tc.skipped) throw_fmt(RJ_ERR_ARG, "column was not uploaded");
            if (t->num_rows == 0) {
                // no rows: a typed column with zero pages
            } else if (tc.type == RJ_VARCHAR) {
                if (vc_directory((int)n.base_table_id, (int)c, t).back() == t->num_rows) {
                    rc.n_pages = tc.vc_pages.size();
                    rc.host_pages.resize(rc.n_pages * PAGE_BYTES);
                    for (uint64_t pg = 0; pg < rc.n_pages; ++pg)
                        memcpy(rc.host_pages.data() + pg * PAGE_BYTES, tc.vc_pages[pg], PAGE_BYTES);
                } else {  // the gather + encode of a join's root, over every row id in order
                    DCol d = table_col(t, (int)c);
                    d.vc_table = (int)n.base_table_id;
                    d.vc_col = (int)c;
                    BufP rowids = ctx->buf(t->num_rows * 4);
                    launch_gather(L, d.ref(), nullptr, t->num_rows, OutStream{rowids->as<uint8_t>(), ST_DENSE32, 0}, nullptr);
                    varchar_root(rowids->as<uint32_t>(), t->num_rows, d, rc);
                }
            } else if (tc.regular) {
                rc.n_pages = tc.n_pages;
                rc.dev_pages = ctx->buf(tc.n_pages * PAGE_BYTES);
                RJ_HIP(hipMemcpyAsync(rc.dev_pages->p, tc.dev_pages, tc.n_pages * PAGE_BYTES,
                                      hipMemcpyDeviceToDevice, ctx->stream));
            } else {  // K1, then the page writer of columns with NULLs
                rc = col_to_result(table_col(t, (int)c), t->num_rows);
            }
            res.cols.push_back(std::move(rc));
        }
    }

    // ------------------------------------------------------------- plan walk
    // execute_impl (reference src/execute.cpp:302-314); children left first (:48-49)
    // `ordered`: every ancestor of this node up to the root is a MAP, which passes the root's order promise
    // down: a sort then orders its rows as at the root (groupings and window nodes always leave theirs in
    // key order)
    Rel node(uint64_t idx, Result* root_res, int depth, bool ordered = false) {
        if (idx >= plan->n_nodes) throw_fmt(RJ_ERR_ARG, "bad node index");
        if (depth > 4096) throw_fmt(RJ_ERR_ARG, "plan too deep (cycle?)");
        const rj_node& n = plan->nodes[idx];
        if (n.kind == RJ_NODE_SCAN) return scan(n);
        const NodeKind* nk = node_kind(n.kind);
        if (nk && nk->children == 1) {
            Rel child = node(n.left, nullptr, depth + 1, n.kind == RJ_NODE_MAP && (root_res != nullptr || ordered));
            switch (n.kind) {
            case RJ_NODE_AGG: return agg(child, n, root_res);
            case RJ_NODE_SELECT: return select(child, n, root_res);
            case RJ_NODE_SORT: return sort(child, n, root_res, ordered);
            case RJ_NODE_GROUP: return group(child, n, root_res);
            case RJ_NODE_WINDOW: return window(child, n, root_res);
            case RJ_NODE_MAP: return map(child, n, root_res);
            }
        }
        if (n.kind == RJ_NODE_SETOP) {  // (two children, no join; the order promise stops here)
            Rel l = node(n.left, nullptr, depth + 1);
            Rel r = node(n.right, nullptr, depth + 1);
            return setop(l, r, n, root_res);
        }
        const JoinKind& K = join_kind(n.kind);
        Rel             l = node(n.left, nullptr, depth + 1);
        Rel             r = node(n.right, nullptr, depth + 1);
        const JoinSpec  js = join_spec(n, ctx->radix_bits_override);
        if (n.kind == RJ_NODE_OUTER) return outer_join(l, r, js, K, root_res);
        if (n.kind == RJ_NODE_FULL) return full_join(l, r, js, K, root_res);
        if (n.kind != RJ_NODE_JOIN) return filter_join(l, r, js, K, root_res);
        return join_core(l, r, js, root_res);
    }

    // -------------------------------------------------------- radix partition
    // (the driver and its pass plan: rj_radix.hip, rj_radix_plan.cpp)
    Parted partition(const PartitionRequest& rq) { return radix_partition(ctx, L, rq); }

    // ---------------------------------------------------------------- join
    struct Side {
        Rel*          rel = nullptr;
        uint64_t      key_col = 0;
        std::set<int> need;       // referenced columns that are not served by the key stream
        int           carry_mode = CARRY_NONE;
        int           carry_col = -1;
        int           CW = 0;
        BufP          stream;     // emitted carry stream
        int           stream_mode = ST_NONE;
        // CARRY_WIDE: the carried columns in record order (a 64-bit one first), then — if any of
        // them has NULLs — one word of validity bits (bit i = wide_cols[i] is non-NULL)
        std::vector<int> wide_cols;
        int              wide = WIDE_NONE;
        int              valid_word = -1;
        BufP             vword;  // the packed validity word per row of the child
        struct WideOut {
            BufP values, valid;
            int  mode = ST_NONE;  // dense values, or — root columns without NULLs — Page images straight away
        };
        std::map<int, WideOut> wide_out;  // per carried column: what k_split_records produced
        // A sharded join's ranks must cut their tuples alike, and whether a column needs a validity
        // word depends on the DATA of a shard: columns that hold NULLs on ANY rank are nullable on
        // every rank (bit c = column c; columns from 64 up count as nullable when `shared` is set)
        uint64_t null_mask = 0;
        bool     shared = false;
        // the optional side of an outer join: every column it delivers can come out NULL (a padded
        // row), whatever the source column holds
        bool     optional = false;
        bool     nullable(int c) const {
            if (optional || rel->cols[c].valid != nullptr) return true;
            return shared && (c >= 64 || ((null_mask >> c) & 1u));
        }
    };
    // which of a relation's (first 64) columns hold NULLs here
    static uint64_t null_columns(const Rel& r) {
        uint64_t m = 0;
        for (size_t c = 0; c < r.cols.size() && c < 64; ++c)
            if (r.cols[c].valid != nullptr) m |= 1ull << c;
        return m;
    }

    static uint64_t pages_for(uint64_t rows, int width) {
        uint64_t rf = width == 4 ? ROWS32 : ROWS64;
        return (rows + rf - 1) / rf;
    }

    // no rows of the declared types: typed columns, at the root with zero pages
    Rel empty_rel(const int32_t* types, uint64_t n_types, Result* root_res) {
        Rel r;
        r.n = 0;
        if (root_res) root_res->num_rows = 0;
        for (uint64_t k = 0; k < n_types; ++k) {
            r.cols.push_back(dense_col(types[k], BufP()));
            if (!root_res) continue;
            ResultColumn rc;
            rc.type = types[k];
            root_res->cols.push_back(std::move(rc));
        }
        return r;
    }
    Rel empty_rel(const rj_node& n, Result* root_res) { return empty_rel(n.out_type, n.n_out, root_res); }
    Rel empty_rel(const JoinSpec& js, Result* root_res) { return empty_rel(js.out_type.data(), js.out_type.size(), root_res); }

    // What a JoinNode decides before any tuple moves: key type, which columns each side
    // must deliver and how they travel (execute_hash_join, reference src/execute.cpp:266-282,
    // and the head of hash_join_omp, :43-83).
    struct JoinState {
        Side     ls, rs;
        bool     build_left = true, is_root = false, f64 = false, need_key_stream = false;
        bool     type_mismatch = false;  // probe key of another type: no row can match (:65-71)
        size_t   lw = 0, rw = 0;
        int      KW = 1;
        uint64_t cap_hint = 0;  // rows the output streams are sized for at the first attempt
        const JoinKind* kind = nullptr;
        // VARCHAR join keys (hash_join_omp<std::string>, src/execute.cpp:278): each side's
        // relation is copied with one extra column — the 64-bit FNV-1a of the key strings —
        // which the join runs on; `rows` remembers where every string sits for the
        // byte-for-byte check of the joined pairs
        bool vkey = false;
        struct VKey {
            Rel            rel;
            BufP           rows, hash, valid;
            const uint8_t* pages = nullptr;
            uint32_t       n_pages = 0;
        } vk[2];  // [0] = left, [1] = right
        Side&    bs() { return build_left ? ls : rs; }
        Side&    ps() { return build_left ? rs : ls; }
    };

    // shared_nulls (sharded joins): {left, right} null_columns() OR-ed over all ranks
    void join_prepare(Rel& left, Rel& right, const JoinSpec& js, bool is_root, JoinState& st, const JoinKind& K,
                      const uint64_t* shared_nulls = nullptr) {
        st.kind = &K;
        const size_t lw = left.cols.size(), rw = right.cols.size();
        st.lw = lw;
        st.rw = rw;
        st.is_root = is_root;
        st.build_left = js.build_left;
        if (js.left_attr >= lw || js.right_attr >= rw)
            throw_fmt(RJ_ERR_ARG, "join: key attr out of range");
        for (size_t k = 0; k < js.out_idx.size(); ++k) {
            if (js.out_idx[k] >= lw + rw) throw_fmt(RJ_ERR_ARG, "join: output attr out of range");
            const DCol& c = js.out_idx[k] < lw ? left.cols[js.out_idx[k]]
                                               : right.cols[js.out_idx[k] - lw];
            if (c.type != js.out_type[k])
                throw_fmt(RJ_ERR_ARG, "join: declared type differs from the child column's type");
        }
        Side &ls = st.ls, &rs = st.rs;
        ls.rel = &left;
        ls.key_col = js.left_attr;
        rs.rel = &right;
        rs.key_col = js.right_attr;
        if (shared_nulls) {
            ls.shared = rs.shared = true;
            ls.null_mask = shared_nulls[0];
            rs.null_mask = shared_nulls[1];
        }
        const DCol& bk = st.bs().rel->cols[st.bs().key_col];
        const DCol& pk = st.ps().rel->cols[st.ps().key_col];
        // KeyType = build side's key type (:271-273)
        if (bk.type < RJ_INT32 || bk.type > RJ_VARCHAR) throw_fmt(RJ_ERR_ARG, "Unsupported join type");
        // probe values of another variant alternative are never valid (:65-71)
        st.type_mismatch = pk.type != bk.type;
        st.vkey = bk.type == RJ_VARCHAR && !st.type_mismatch;
        st.KW = bk.type == RJ_INT32 ? 1 : 2;
        st.f64 = bk.type == RJ_FP64;
        // matching keys are bit-identical on both sides (FP64 included: bit-pattern equality,
        // see SrcLoader::key2), so one emitted key stream serves either side's key column.
        // A semi / anti join emits the preserved side's own key — through the key stream unless
        // its type is not the key type (no key is read then) or ANTI may emit rows whose key is
        // NULL (the stream has no validity): then the key column travels as a payload column.
        // An outer join emits unmatched rows as ANTI does, so the preserved key follows ANTI's rule;
        // the optional side's key column is NULL in those rows and never comes from the key stream:
        // it travels as one of that side's payload columns.
        const bool key_stream_ok =
            K.node == RJ_NODE_JOIN ||
            (!st.type_mismatch && !(K.emits_unmatched && st.ps().rel->cols[st.ps().key_col].valid));
        st.bs().optional = K.build_optional;
        st.ps().optional = K.probe_optional;  // (both: neither side's key column comes from the key stream)
        // Which child columns must each side deliver?
        for (size_t k = 0; k < js.out_idx.size(); ++k) {
            bool  is_left = js.out_idx[k] < lw;
            Side& s = is_left ? ls : rs;
            int   c = (int)(is_left ? js.out_idx[k] : js.out_idx[k] - lw);
            if ((uint64_t)c == s.key_col && !st.vkey && key_stream_ok && !s.optional)
                st.need_key_stream = true;
            else
                s.need.insert(c);  // (a VARCHAR key column is gathered like any other column)
        }
        for (Side* s : {&ls, &rs}) {
            if (st.vkey) {  // both row indices are needed for the string comparison of the pairs
                s->carry_mode = CARRY_ROWIDX;
                s->CW = 1;
            } else if (s->need.empty()) {
                s->carry_mode = CARRY_NONE;
                s->CW = 0;
            } else if (s->need.size() == 1 && !s->nullable(*s->need.begin())) {
                s->carry_mode = CARRY_COLUMN;
                s->carry_col = *s->need.begin();
                s->CW = s->rel->cols[s->carry_col].width / 4;
            } else if (plan_wide_carry(*s, st.KW)) {
                s->carry_mode = CARRY_WIDE;
            } else {
                s->carry_mode = CARRY_ROWIDX;
                s->CW = 1;
            }
        }
        st.cap_hint = std::max(left.n, right.n);
    }

    // Can the columns a side must deliver travel WITH the key (reference src/execute.cpp:236-242
    // copies any column list per output row; here up to MAX_WORDS - KW carry words do the same
    // without a row index to gather through afterwards)?  Layouts: two or three 32-bit words, or
    // a 64-bit column followed by one 32-bit word; a validity word counts as a 32-bit word.
    // honour_switch = false: a caller without a row-index fallback (the aggregation) plans the
    // layout whatever the wide-carry tuning switch says
    bool plan_wide_carry(Side& s, int KW, bool honour_switch = true) {
        if ((honour_switch && !ctx->tune.wide_carry) || s.need.empty()) return false;
        int  words = 0, n64 = 0;
        bool any_null = false;
        for (int c : s.need) {
            const DCol& col = s.rel->cols[c];
            if (col.width != 4 && col.width != 8) return false;
            words += col.width / 4;
            n64 += col.width == 8;
            any_null = any_null || s.nullable(c);
        }
        if (any_null) ++words;
        if (words < 2 || words > MAX_WORDS - KW || n64 > 1 || (n64 == 1 && words != 3)) return false;
        s.wide_cols.clear();
        for (int c : s.need)
            if (s.rel->cols[c].width == 8) s.wide_cols.push_back(c);
        for (int c : s.need)
            if (s.rel->cols[c].width == 4) s.wide_cols.push_back(c);
        s.wide = n64 ? WIDE_64_32 : WIDE_32S;
        s.valid_word = any_null ? words - 1 : -1;
        s.CW = words;
        return true;
    }

    // validity bits of a wide carry's columns, one word per row (k_pack_validity); call once
    // per join before the side's tuples are formed
    void prepare_wide(Side& s) {
        if (s.carry_mode != CARRY_WIDE || s.valid_word < 0 || s.rel->n == 0) return;
        const uint8_t* v[3] = {nullptr, nullptr, nullptr};
        for (size_t i = 0; i < s.wide_cols.size() && i < 3; ++i) v[i] = s.rel->cols[s.wide_cols[i]].valid;
        s.vword = ctx->buf(s.rel->n * 4);
        launch_pack_validity(L, v[0], v[1], v[2], (uint32_t)s.rel->n, s.vword->as<uint32_t>());
    }

    // radix bit plan from the build cardinality; `top_bits_taken` high hash bits are constant
    // on this rank (a sharded join's rank digit): the plan stays below them
    uint32_t join_bits(const JoinSpec& js, uint64_t build_n, uint32_t top_bits_taken = 0) {
        uint32_t bits = js.forced_bits > 0 ? (uint32_t)js.forced_bits
                                           : ceil_log2((build_n + JN_TARGET_BUILD - 1) / JN_TARGET_BUILD);
        // a third pass costs 20 B/tuple more than slightly fuller tables: stay at two passes
        // (2 * PT_MAXBITS bits) while the mean build partition still fits the LDS table with
        // a margin (rare larger partitions are joined in table-sized chunks anyway)
        if (js.forced_bits <= 0 && bits > 2 * PT_MAXBITS &&
            (build_n >> (2 * PT_MAXBITS)) <= (uint64_t)(JN_RMAX * 0.95))
            bits = 2 * PT_MAXBITS;
        // (at most 21: three passes of 7 bits — what 2^32 build rows ask for; more partitions than that
        // and the join's launch would exceed 2^32 threads.  A larger forced value is clamped.)
        bits = std::min<uint32_t>(std::max<uint32_t>(bits, 1), 21);
        if (top_bits_taken && bits > 32 - top_bits_taken) bits = 32 - top_bits_taken;
        return bits;
    }

    TupleSrc make_src(const JoinState& st, const Side& s, const JoinSpec& js) {
        TupleSrc src{};
        src.key = s.rel->cols[s.key_col].ref();
        src.n_rows = (uint32_t)s.rel->n;
        src.carry_mode = s.carry_mode;
        if (s.carry_mode == CARRY_COLUMN) {
            src.carry = s.rel->cols[s.carry_col].ref();
            // a base table's row-id column (VARCHAR stand-in) IS the row index
            if (src.carry.kind == COL_IOTA) src.carry_mode = CARRY_ROWIDX;
        }
        if (s.carry_mode == CARRY_WIDE) {
            ColRef refs[3] = {};
            size_t k = 0;
            for (int c : s.wide_cols) refs[k++] = s.rel->cols[c].ref();
            if (s.valid_word >= 0)
                refs[k++] = ColRef{ptr<uint8_t>(s.vword), nullptr, COL_DENSE, 4};
            src.wide = s.wide;
            src.carry = refs[0];
            src.carry2 = refs[1];
            src.carry3 = refs[2];
        }
        src.key_f64 = st.f64 ? 1 : 0;
        src.prehashed = js.prehashed ? 1 : 0;
        return src;
    }

    // ------------------------------------------------- the probe step of a join node
    // What the five kinds share, each written once: whether the node is partitioned at all
    // (broadcast_form), the co-partitions and their heavy-task list (CoParts), and the output
    // protocol (emit_with_retry).  A kind's own function keeps its refusals and early returns, its
    // parameter struct and the kernels it launches per attempt.

    // A build side that fits one LDS table is not partitioned: every workgroup builds the same
    // table and streams a slice of the probe child past it (the *_bcast kernels).  The kinds that
    // get here with an empty build side or with keys of another type (they emit rows without a
    // partner) need no table at all, which the broadcast kernels handle.
    bool broadcast_form(JoinState& st, const JoinSpec& js) const {
        const uint64_t nb = st.bs().rel->n;
        return (nb <= (uint64_t)JN_RMAX && js.forced_bits <= 0 && !js.prehashed && ctx->tune.bcast != 0) || nb == 0 ||
               st.type_mismatch;
    }
    // workgroups that stride over `rows` rows in chunks of JN_SUB
    uint32_t stride_grid(uint64_t rows) const {
        return (uint32_t)std::min<uint64_t>((rows + JN_SUB - 1) / JN_SUB, (uint64_t)ctx->compute_units() * 8);
    }

    // Both sides of a partitioned node, cut with the same bit plan, and the probe partitions that
    // are split into tasks (k_heavy_tasks).  A ShardedExec fills B and P itself, from the exchange.
    struct CoParts {
        Parted   B, P;
        BufP     tasks;  // [max_tasks][3]
        uint32_t max_tasks = 0;
    };
    // counters (optional, from zeroed_counters()): either side's first pass may run speculatively (PartitionRequest::
    // spec_flag), with the node's two flag words; emit_with_retry then sees them with the row count, and
    // repartition_exact() is what its caller does about a flag that is set
    // spec2_ok: the node's kernels read a partition through Parted::off_shift, so the last pass may be speculative as well
    CoParts partition_sides(JoinState& st, const JoinSpec& js, uint32_t bits, const BufP* counters = nullptr, bool spec2_ok = false) {
        CoParts        cp;
        const TupleSrc sb = make_src(st, st.bs(), js), sp = make_src(st, st.ps(), js);
        uint32_t*      fl = counters ? (*counters)->as<uint32_t>() + 4 : nullptr;
        PartitionRequest rb = PartitionRequest::columns(sb, st.KW, st.bs().CW, bits), rp = PartitionRequest::columns(sp, st.KW, st.ps().CW, bits);
        rb.spec_flag = fl;
        rp.spec_flag = fl ? fl + 1 : nullptr;
        rb.spec2_ok = rp.spec2_ok = spec2_ok;
        cp.B = partition(rb);
        cp.P = partition(rp);
        return cp;
    }
    // A speculative pass (the first, or an inner join's last) found a sub-range too small (flag_b / flag_p: on which side).  What the node has
    // produced since is thrown away: that side is partitioned again, with its histogram, the heavy tasks are listed
    // again (which zeroes the row cursor) and the flags are cleared.  The caller then points its kernel parameters
    // at the new partitions and runs the probe again.
    int  spec_fallbacks = 0;
    void repartition_exact(JoinState& st, const JoinSpec& js, uint32_t bits, CoParts& cp, const BufP& counters, bool flag_b,
                           bool flag_p) {
        ++spec_fallbacks;
        if (ctx->tune.diag >= 1)
            fprintf(stderr, "[rj diag] %s: a speculative pass overflowed (build side %d, probe side %d): exact partition again (fallback %d of this plan)\n",
                    st.kind->name, (int)flag_b, (int)flag_p, spec_fallbacks);
        if (flag_b) {
            const TupleSrc sb = make_src(st, st.bs(), js);
            cp.B = Parted();  // (its arrays go back to the block cache first)
            cp.B = partition(PartitionRequest::columns(sb, st.KW, st.bs().CW, bits));  // (no flag word: both passes exact)
        }
        if (flag_p) {
            const TupleSrc sp = make_src(st, st.ps(), js);
            cp.P = Parted();
            cp.P = partition(PartitionRequest::columns(sp, st.KW, st.ps().CW, bits));
        }
        RJ_HIP(hipMemsetAsync(counters->as<uint32_t>() + 4, 0, 8, ctx->stream));
        cp.tasks = BufP();
        heavy_tasks(cp, counters);
    }
    // heavy probe partitions -> task list; zeroes all 16 bytes of `counters` on the way
    void heavy_tasks(CoParts& cp, const BufP& counters) {
        cp.max_tasks = (uint32_t)(2 * (cp.P.n_tuples / JN_HEAVY) + 2);
        cp.tasks = ctx->buf((uint64_t)cp.max_tasks * 12);
        launch_heavy_tasks_zeroed(cp.B, cp.P, cp.tasks, counters, cp.max_tasks);
    }
    CoParts co_partition(JoinState& st, const JoinSpec& js, uint32_t bits, const BufP& counters) {
        CoParts cp = partition_sides(st, js, bits, &counters);
        heavy_tasks(cp, counters);
        return cp;
    }
    // [0..7] out cursor (u64), [8..11] n_heavy, [12..15] the aggregation's overflow flag, [16..19] / [20..23] a join's
    // build / probe side: a speculative pass of it (the first, or the last) did not fit (SpecParams::flag)
    static constexpr size_t COUNTER_BYTES = 32;
    BufP zeroed_counters() {
        BufP counters = ctx->buf(COUNTER_BYTES);
        RJ_HIP(hipMemsetAsync(counters->p, 0, COUNTER_BYTES, ctx->stream));
        return counters;
    }
    // the fields every partitioned probe kernel's parameters hold under the same names
    template <class Params>
    static void set_heavy(Params& p, const CoParts& cp, const BufP& counters, uint32_t bits) {
        p.NP = cp.B.NP;
        p.radix_bits = bits;
        p.heavy_tasks = cp.tasks->as<uint32_t>();
        p.n_heavy = counters->as<uint32_t>() + 2;
        p.heavy_grid = cp.max_tasks;
    }
    static void set_parts(OuterParams& op, const CoParts& cp, const BufP& counters, uint32_t bits) {
        set_heavy(op, cp, counters, bits);
        op.Bw = cp.B.w;
        op.Pw = cp.P.w;
        op.offB = cp.B.off->as<uint32_t>();
        op.offP = cp.P.off->as<uint32_t>();
        op.packB = cp.B.packed ? 1 : 0;
        op.aosB = cp.B.aos3 ? 1 : 0;
        op.packP = cp.P.packed ? 1 : 0;
        op.aosP = cp.P.aos3 ? 1 : 0;
    }

    static OutStream out_stream(const BufP& b, int mode) { return OutStream{ptr<uint8_t>(b), mode, 0}; }
    static OutStream out_stream(const Side& s) { return out_stream(s.stream, s.stream_mode); }
    // rows the streams of a first attempt hold when the result may exceed `rows`
    static uint64_t first_cap(uint64_t rows) { return std::min<uint64_t>(rows + 1024, 0xfffffff0ull); }

    struct Emitted {
        uint64_t        nrows = 0;
        BufP            key_stream;
        int             key_mode = ST_NONE;
        std::set<void*> finished;  // paged buffers that already got their headers
    };
    // The output protocol of every kind: streams for `cap` rows; the kernels count every row they
    // produce on the device (counters[0..7]) and write only what fits; a count beyond `cap` runs
    // the attempt once more with streams of exactly that size.  A kind whose first capacity is a
    // bound (JoinKind::attempts == 1) never reruns.  `launch(key, cap)` enqueues one attempt; the
    // carry streams are st.ls.stream / st.rs.stream.  Page headers of the streams the probe wrote
    // straight into Page images are made on the device from the device-side row count, so nothing
    // waits for the read-back.  (FULL has no such stream: both of its sides are optional, so both
    // carries are dense records or row ids and no key stream exists; finish_paged_streams then
    // finds nothing and no k_finish_streams is launched.)
    // `respec(flag_b, flag_p)` (optional; `counters` then come from zeroed_counters()): the sides were partitioned
    // with partition_sides(.., &counters).  The flag words travel with the row count; when one is set the attempt
    // counted rows of truncated partitions, so it is looked at before the count: respec() partitions again
    // (repartition_exact) and the node starts over at its first capacity.
    template <class LaunchFn>
    Emitted emit_with_retry(JoinState& st, const BufP& counters, uint64_t cap, LaunchFn&& launch,
                            const std::function<void(bool, bool)>& respec = nullptr) {
        const JoinKind& K = *st.kind;
        Emitted         e;
        const uint64_t  cap0 = cap;
        e.key_mode = st.need_key_stream ? stream_mode_of(st.is_root, st.KW * 4, true) : ST_NONE;
        for (int attempt = 1;; ++attempt) {
            e.key_stream = e.key_mode != ST_NONE ? ctx->buf(stream_bytes(e.key_mode, cap)) : BufP();
            for (Side* s : {&st.ls, &st.rs})
                s->stream = s->stream_mode != ST_NONE ? ctx->buf(stream_bytes(s->stream_mode, cap)) : BufP();
            // (a kind with a single attempt has just zeroed the cursor with the rest of the counters)
            if (K.attempts > 1) RJ_HIP(hipMemsetAsync(counters->p, 0, 8, ctx->stream));
            launch(out_stream(e.key_stream, e.key_mode), cap);
            e.finished.clear();
            finish_paged_streams(st, e, counters, cap);
            unsigned long long h = 0;
            if (respec) {
                uint32_t hw[6] = {};
                read_back(hw, counters->p, sizeof hw);
                if (hw[4] | hw[5]) {
                    respec(hw[4] != 0, hw[5] != 0);
                    cap = cap0;
                    attempt = 0;
                    continue;
                }
                h = (unsigned long long)hw[0] | ((unsigned long long)hw[1] << 32);
            } else {
                read_back(&h, counters->p, 8);
            }
            e.nrows = h;
            if (e.nrows <= cap) return e;
            if (K.attempts == 1)
                throw_fmt(RJ_ERR_DEVICE, "%s emitted %llu rows out of %llu", K.name, h, (unsigned long long)cap);
            if (e.nrows > 0xfffffff0ull) throw_fmt(RJ_ERR_UNSUPPORTED, "%s result exceeds 2^32 rows (%llu)", K.name, h);
            if (attempt == K.attempts) throw_fmt(RJ_ERR_DEVICE, "%s output overflowed twice", K.name);
            cap = e.nrows;  // exact size, run the probe again
        }
    }

    // execute_hash_join + hash_join_omp (reference src/execute.cpp:43-282) on one device
    Rel join_core(Rel& left, Rel& right, const JoinSpec& js, Result* root_res) {
        // with an empty child the reference returns {} before looking at anything (:50)
        if (left.n == 0 || right.n == 0) return empty_rel(js, root_res);
        JoinState st;
        join_prepare(left, right, js, root_res != nullptr, st, join_kind(RJ_NODE_JOIN));
        if (st.type_mismatch) return empty_rel(js, root_res);
        if (st.vkey) hash_varchar_keys(st);
        prepare_wide(st.ls);
        prepare_wide(st.rs);
        Side&          bs = st.bs();
        Side&          ps = st.ps();
        const uint32_t bits = join_bits(js, bs.rel->n, js.top_bits_taken);
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] join build=%llu probe=%llu bits=%u cw=%d/%d\n",
                    (unsigned long long)bs.rel->n, (unsigned long long)ps.rel->n, bits, bs.CW, ps.CW);
        if (broadcast_form(st, js)) return join_finish(st, js, nullptr, bits, root_res);
        BufP    counters = zeroed_counters();
        // (the last pass may be speculative too where k_join reads {begin, end} pairs: rj_join.hip, PAIRS)
        const bool pairs = st.KW == 1 && bs.CW >= 1 && bs.CW <= 2 && ps.CW >= 1 && ps.CW <= 2;
        CoParts cp = partition_sides(st, js, bits, &counters, pairs);
        return join_finish(st, js, &cp, bits, root_res, counters);
    }

    // Build + probe of an inner join over co-partitioned tuples (cp->B / cp->P; nullptr = broadcast
    // join straight from the children's columns), output streams, late materialisation, result pages.
    // (spec_counters: the zeroed counters the sides were partitioned with, if their first passes may have been speculative)
    Rel join_finish(JoinState& st, const JoinSpec& js, CoParts* cp, uint32_t bits, Result* root_res,
                    const BufP& spec_counters = BufP()) {
        Side &    bs = st.bs(), &ps = st.ps();
        const int KW = st.KW;
        // (not zeroed here: heavy_tasks() zeroes all of it, and the broadcast form uses the cursor
        // alone, which every attempt resets)
        BufP counters = spec_counters ? spec_counters : ctx->buf(COUNTER_BYTES);  // (see zeroed_counters)
        if (cp) heavy_tasks(*cp, counters);
        std::function<void(bool, bool)> respec;
        if (cp && spec_counters && (cp->B.spec || cp->P.spec))
            respec = [&](bool fb, bool fpr) { repartition_exact(st, js, bits, *cp, counters, fb, fpr); };
        plan_carry_streams(st);
        Emitted e = emit_with_retry(st, counters, first_cap(st.cap_hint), [&](const OutStream& key, uint64_t cap) {
            if (!cp) {
                BcastParams bp{};
                bp.R = make_src(st, bs, js);
                bp.S = make_src(st, ps, js);
                bp.key = key;
                bp.bc = out_stream(bs);
                bp.pc = out_stream(ps);
                bp.out_cursor = counters->as<unsigned long long>();
                bp.out_cap = cap;
                launch_join_bcast(L, KW, bs.CW, ps.CW, bp, stride_grid(ps.rel->n));
                return;
            }
            const Parted &PB = cp->B, &PP = cp->P;
            JoinParams    jp{};
            set_heavy(jp, *cp, counters, bits);
            jp.R = PB.w;
            jp.S = PP.w;
            jp.packR = PB.packed ? 1 : 0;
            jp.packS = PP.packed ? 1 : 0;
            jp.aosR = PB.aos3 ? 1 : 0;
            jp.aosS = PP.aos3 ? 1 : 0;
            jp.offR = PB.off->as<uint32_t>();
            jp.offS = PP.off->as<uint32_t>();
            jp.off_pairs = PB.off_shift | (PP.off_shift << 1);
            if (jp.off_pairs && !(KW == 1 && bs.CW >= 1 && bs.CW <= 2 && ps.CW >= 1 && ps.CW <= 2))
                throw_fmt(RJ_ERR_DEVICE, "join: {begin, end} pairs for a shape whose kernel does not read them");
            jp.n_pass = (uint32_t)PB.pbits.size();
            for (size_t i = 0; i < PB.pbits.size() && i < 4; ++i) jp.pass_bits[i] = PB.pbits[i];
            jp.key = key;
            jp.bc = out_stream(bs);
            jp.pc = out_stream(ps);
            jp.out_cursor = counters->as<unsigned long long>();
            jp.out_cap = cap;
            BufP diag;
            if (ctx->tune.diag) {
                diag = ctx->buf(16 * 8);
                RJ_HIP(hipMemsetAsync(diag->p, 0, 16 * 8, ctx->stream));
                jp.diag = diag->as<unsigned long long>();
            }
            // one launch: heavy-task workgroups first, then one workgroup per `ppw` partitions
            const uint32_t ppw = join_partitions_per_workgroup(KW, bs.CW, jp);
            launch_join(L, KW, bs.CW, ps.CW, jp, cp->max_tasks + (PB.NP + ppw - 1) / ppw);
            if (diag) {
                unsigned long long hd[16];
                read_back(hd, diag->p, sizeof hd);
                static const char* names[] = {"loads issued", "table clear", "build", "count/probe",
                                              "prefix+barrier", "reserve", "emit"};
                double tot = 0;
                for (int i = 0; i < 7; ++i) tot += (double)hd[i];
                fprintf(stderr, "[rj diag] join phases (cycles of thread 0, summed over %u workgroups):\n", PB.NP);
                for (int i = 0; i < 7; ++i)
                    fprintf(stderr, "[rj diag]   %-16s %6.1f %%  %8.0f cyc/wg\n", names[i],
                            100.0 * hd[i] / tot, (double)hd[i] / PB.NP);
            }
        }, respec);
        if (st.vkey && e.nrows) e.nrows = verify_varchar_pairs(st, e.nrows);
        return join_assemble(st, js, e, root_res);
    }

    // Semi / anti join (RJ_NODE_SEMI / RJ_NODE_ANTI, semantics in rj.h): the build side is the
    // filter side and carries nothing, the probe side is preserved; every preserved row that has
    // (SEMI) or has not (ANTI) a partner comes out once, with the preserved side's columns only.
    Rel filter_join(Rel& left, Rel& right, const JoinSpec& js, const JoinKind& K, Result* root_res) {
        const bool   anti = K.node == RJ_NODE_ANTI;
        Rel&         fil = js.build_left ? left : right;
        Rel&         pre = js.build_left ? right : left;
        const size_t lw = left.cols.size();
        for (uint64_t o : js.out_idx)
            if (o < lw + right.cols.size() && (o < lw) == js.build_left)
                throw_fmt(RJ_ERR_ARG, "%s: output attr %llu names a column of the filter side", K.name,
                          (unsigned long long)o);
        const uint64_t fattr = js.build_left ? js.left_attr : js.right_attr;
        if (fattr < fil.cols.size() && fil.cols[fattr].type == RJ_VARCHAR)
            throw_fmt(RJ_ERR_UNSUPPORTED, "%s on a VARCHAR key", K.name);
        if (pre.n == 0 || (!anti && fil.n == 0)) return empty_rel(js, root_res);
        JoinState st;
        join_prepare(left, right, js, root_res != nullptr, st, K);
        if (st.type_mismatch && !anti) return empty_rel(js, root_res);
        Side&     fs = st.bs();
        Side&     ps = st.ps();
        const int KW = st.KW;
        prepare_wide(ps);
        plan_carry_streams(st);
        const bool     bcast = broadcast_form(st, js);  // (an empty filter side, keys of another type: every row misses)
        const uint32_t bits = join_bits(js, fs.rel->n);
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] %s filter=%llu preserved=%llu %s bits=%u cw=%d\n", K.name,
                    (unsigned long long)fs.rel->n, (unsigned long long)ps.rel->n, bcast ? "broadcast" : "partitioned",
                    bits, ps.CW);

        FilterParams fp{};
        fp.anti = anti ? 1 : 0;
        fp.keyless = st.type_mismatch ? 1 : 0;
        fp.P = make_src(st, ps, js);
        if (bcast && !fp.keyless) fp.F = make_src(st, fs, js);
        BufP counters = zeroed_counters();
        fp.out_cursor = counters->as<unsigned long long>();
        CoParts cp;
        auto    bind_parts = [&]() {
            set_heavy(fp, cp, counters, bits);
            fp.Fw = cp.B.w;
            fp.Pw = cp.P.w;
            fp.offF = cp.B.off->as<uint32_t>();
            fp.offP = cp.P.off->as<uint32_t>();
            fp.packP = cp.P.packed ? 1 : 0;
            fp.aosP = cp.P.aos3 ? 1 : 0;
        };
        if (!bcast) {
            // both sides partitioned as an inner join's would be; the filter side carries nothing
            cp = co_partition(st, js, bits, counters);
            bind_parts();
        }
        std::function<void(bool, bool)> respec;
        if (cp.B.spec || cp.P.spec)
            respec = [&](bool fb, bool fpr) {
                repartition_exact(st, js, bits, cp, counters, fb, fpr);
                bind_parts();
            };
        // the output never holds more rows than the preserved side: streams of that size, no retry
        Emitted e = emit_with_retry(st, counters, ps.rel->n, [&](const OutStream& key, uint64_t cap) {
            fp.key = key;
            fp.pc = out_stream(ps);
            fp.out_cap = cap;
            if (bcast) {
                launch_filter_bcast(L, KW, ps.CW, fp, stride_grid(ps.rel->n));
            } else {
                launch_filter_join(L, KW, ps.CW, fp, cp.max_tasks + cp.B.NP);
                // the rows the first radix pass dropped: NULL keys, FP64 NaN keys
                if (anti && (fp.P.key.valid || fp.P.key_f64))
                    launch_filter_nullkeys(L, KW, ps.CW, fp, stride_grid(ps.rel->n));
            }
        }, respec);
        return join_assemble(st, js, e, root_res);
    }

    // Outer join (RJ_NODE_OUTER, semantics in rj.h): the build side is the OPTIONAL side, the probe
    // side is preserved.  The inner join's rows plus one row per preserved row without a partner,
    // whose optional-side columns are NULL.  Both sides are partitioned as an inner join's are
    // (or not at all: broadcast); one kernel family emits both halves.  NULL travels in-band in the
    // optional side's carry (OuterParams), so that side never uses CARRY_COLUMN.
    Rel outer_join(Rel& left, Rel& right, const JoinSpec& js, const JoinKind& K, Result* root_res) {
        Rel&           opt = js.build_left ? left : right;
        Rel&           pre = js.build_left ? right : left;
        const uint64_t oattr = js.build_left ? js.left_attr : js.right_attr;
        if (oattr < opt.cols.size() && opt.cols[oattr].type == RJ_VARCHAR)
            throw_fmt(RJ_ERR_UNSUPPORTED, "%s on a VARCHAR key", K.name);
        if (pre.n == 0) return empty_rel(js, root_res);
        JoinState st;
        join_prepare(left, right, js, root_res != nullptr, st, K);
        return outer_probe(st, js, root_res);
    }

    // Full outer join (RJ_NODE_FULL, semantics in rj.h): an outer join whose probed side is
    // optional too.  The probe kernels are the outer join's with one addition: every build tuple
    // that matched gets its bit set in `flags` (HBM, one bit per build tuple, zeroed once per
    // node; a rerun sets the same bits again).  A second phase in the same stream then emits the
    // build tuples whose bit stayed clear, and the build rows the table never saw (NULL / NaN
    // keys), with the probed side's carry padded.  NULL travels in-band in BOTH carries.
    Rel full_join(Rel& left, Rel& right, const JoinSpec& js_in, const JoinKind& K, Result* root_res) {
        for (int side = 0; side < 2; ++side) {
            const Rel&     r = side == 0 ? left : right;
            const uint64_t a = side == 0 ? js_in.left_attr : js_in.right_attr;
            if (a < r.cols.size() && r.cols[a].type == RJ_VARCHAR)
                throw_fmt(RJ_ERR_UNSUPPORTED, "%s on a VARCHAR key", K.name);
        }
        // what the node may output is a property of the plan, not of the data: a malformed node and
        // a VARCHAR output column are refused whatever the children hold
        if (left.n == 0 && right.n == 0) {
            JoinState chk;
            join_prepare(left, right, js_in, root_res != nullptr, chk, K);
            refuse_varchar_outputs(chk);
            return empty_rel(js_in, root_res);
        }
        // build_left is a hint: an empty probed side would leave the probe kernels without work
        // and the partitioner without tuples, so the empty child is the one that is built
        JoinSpec js = js_in;
        if ((js.build_left ? right : left).n == 0) js.build_left = !js.build_left;
        JoinState st;
        join_prepare(left, right, js, root_res != nullptr, st, K);
        return outer_probe(st, js, root_res);
    }

    // a VARCHAR column of an optional side cannot come out
    static void refuse_varchar_outputs(JoinState& st) {
        for (Side* s : {&st.ls, &st.rs})
            for (int c : s->need) {
                if (!s->optional || s->rel->cols[c].type != RJ_VARCHAR) continue;
                if (st.kind->probe_optional)
                    throw_fmt(RJ_ERR_UNSUPPORTED,
                              "full outer join: a VARCHAR column in the output is not supported (%s child column %d)",
                              s == &st.ls ? "left" : "right", c);
                throw_fmt(RJ_ERR_UNSUPPORTED,
                          "outer join: a VARCHAR column of the optional side in the output is not supported "
                          "(child column %d)", c);
            }
    }

    // What OUTER and FULL do once the node is prepared.  FULL's parameters hold an outer join's.
    Rel outer_probe(JoinState& st, const JoinSpec& js, Result* root_res) {
        const bool full = st.kind->probe_optional;
        Side&      bs = st.bs();
        Side&      ps = st.ps();
        const int  KW = st.KW;
        refuse_varchar_outputs(st);
        prepare_wide(bs);
        prepare_wide(ps);
        plan_carry_streams(st);
        const bool     bcast = broadcast_form(st, js);  // (no table at all: every row comes out padded)
        const uint32_t bits = join_bits(js, bs.rel->n);
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] %s %s=%llu %s=%llu %s bits=%u cw=%d/%d\n", st.kind->name, full ? "built" : "optional",
                    (unsigned long long)bs.rel->n, full ? "probed" : "preserved", (unsigned long long)ps.rel->n,
                    bcast ? "broadcast" : "partitioned", bits, bs.CW, ps.CW);

        FullParams   fp{};
        OuterParams& op = fp.o;
        op.keyless = st.type_mismatch ? 1 : 0;
        op.pad_bc = bs.carry_mode == CARRY_ROWIDX ? OUTER_NO_ROW : 0u;
        op.P = make_src(st, ps, js);
        // (FULL, keyless: the build side's key is never read, its carry is)
        if (full || !op.keyless) op.B = make_src(st, bs, js);
        BufP counters = zeroed_counters();
        op.out_cursor = counters->as<unsigned long long>();
        CoParts cp;
        if (!bcast) {
            cp = co_partition(st, js, bits, counters);
            set_parts(op, cp, counters, bits);
        }
        BufP flags;
        if (full) {
            fp.pad_pc = ps.carry_mode == CARRY_ROWIDX ? OUTER_NO_ROW : 0u;
            // one matched bit per build tuple (partitioned: by index in cp.B's arrays; broadcast: by
            // row of the built child), whole words, one spare word for the round that ends unaligned
            const uint64_t flag_bytes = ((bcast ? (uint64_t)JN_RMAX : cp.B.n_tuples) / 32 + 2) * 4;
            flags = ctx->buf(flag_bytes);
            RJ_HIP(hipMemsetAsync(flags->p, 0, flag_bytes, ctx->stream));
            fp.flags = flags->as<uint32_t>();
            fp.use_flags = bcast ? 1 : 0;
        }
        std::function<void(bool, bool)> respec;
        if (cp.B.spec || cp.P.spec)
            respec = [&](bool fb, bool fpr) {
                repartition_exact(st, js, bits, cp, counters, fb, fpr);
                set_parts(op, cp, counters, bits);
                // (FULL: the matched bits of the attempt that is thrown away)
                if (flags) RJ_HIP(hipMemsetAsync(flags->p, 0, ((cp.B.n_tuples) / 32 + 2) * 4, ctx->stream));
            };
        const uint32_t probe_grid = stride_grid(ps.rel->n), build_grid = stride_grid(bs.rel->n);
        // OUTER holds at least the preserved rows, FULL may hold every row of both sides, and
        // dup x dup may exceed either
        const uint64_t rows0 = std::max(st.cap_hint, full ? bs.rel->n + ps.rel->n : ps.rel->n);
        Emitted e = emit_with_retry(st, counters, first_cap(rows0), [&](const OutStream& key, uint64_t cap) {
            op.key = key;  // (FULL: none, neither side's key column comes from a key stream)
            op.bc = out_stream(bs);
            op.pc = out_stream(ps);
            op.out_cap = cap;
            // the rows the first radix pass dropped: NULL keys, FP64 NaN keys
            const bool probe_dropped = !bcast && (op.P.key.valid || op.P.key_f64);
            if (!full) {
                if (bcast)
                    launch_outer_bcast(L, KW, bs.CW, ps.CW, op, probe_grid);
                else
                    launch_outer_join(L, KW, bs.CW, ps.CW, op, cp.max_tasks + cp.B.NP);
                if (probe_dropped) launch_outer_nullkeys(L, KW, ps.CW, op, probe_grid);
            } else if (bcast) {
                launch_full_bcast(L, KW, bs.CW, ps.CW, fp, probe_grid);
                // unmatched build rows and build rows without a usable key, in one sweep
                launch_full_buildrows(L, KW, bs.CW, fp, build_grid);
            } else {
                launch_full_join(L, KW, bs.CW, ps.CW, fp, cp.max_tasks + cp.B.NP);
                launch_full_unmatched(L, KW, bs.CW, fp, build_grid);
                if (probe_dropped) launch_outer_nullkeys(L, KW, ps.CW, op, probe_grid);
                if (op.B.key.valid || op.B.key_f64) launch_full_buildrows(L, KW, bs.CW, fp, build_grid);
            }
        }, respec);
        return join_assemble(st, js, e, root_res);
    }

    // ---------------------------------------------------------------- aggregation
    // RJ_NODE_AGG (semantics in rj.h): GROUP BY one key column with COUNT / SUM / MIN / MAX.  ONE
    // relation is partitioned — the key plus the distinct aggregated columns as its carry — and
    // k_agg_parts aggregates every partition in an LDS table.  Partitions above JN_HEAVY tuples are
    // cut into tasks whose groups meet in a merge table in HBM, as does the group of the NULL-key
    // rows, which the first radix pass drops; k_agg_emit turns that table into rows.  The group
    // count is bounded by the child's rows, so the output arrays never overflow: one attempt.
    struct AggOut {
        uint32_t func;
        int      col;   // child column
        int      slot;  // index among the carried columns, -1 = none (KEY, COUNT(*))
    };
    uint32_t agg_bits(uint64_t rows) const {
        uint32_t bits = ctx->radix_bits_override > 0 ? (uint32_t)ctx->radix_bits_override
                                                     : ceil_log2((rows + AGG_TARGET - 1) / AGG_TARGET);
        return std::min<uint32_t>(std::max<uint32_t>(bits, 1), 21);
    }
    Rel agg(Rel& child, const rj_node& n, Result* root_res) {
        const size_t cw = child.cols.size();
        if (n.left_attr >= cw) throw_fmt(RJ_ERR_ARG, "aggregation: key attr out of range");
        const DCol& kc = child.cols[n.left_attr];
        if (kc.type != RJ_INT32 && kc.type != RJ_INT64)
            throw_fmt(RJ_ERR_UNSUPPORTED, "aggregation on %s key: group keys are INT32 or INT64",
                      kc.type == RJ_FP64 ? "an FP64" : "a VARCHAR");
        Side s;
        s.rel = &child;
        s.key_col = n.left_attr;
        std::vector<AggOut> outs;
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint32_t func = RJ_AGG_FUNC(n.out_idx[k]);
            const uint64_t col = RJ_AGG_COL(n.out_idx[k]);
            const int32_t  type = n.out_type[k];
            if (func == RJ_AGG_FSUM) throw_fmt(RJ_ERR_ARG, "aggregation: RJ_AGG_FSUM is RJ_NODE_GROUP's, this kind has no FP64 sum");
            if (func > RJ_AGG_MAX) throw_fmt(RJ_ERR_ARG, "aggregation: unknown function code %u", func);
            int32_t expect = RJ_INT64;
            if (func == RJ_AGG_COUNT_STAR) {
                if (col != 0) throw_fmt(RJ_ERR_ARG, "aggregation: COUNT(*) takes no column");
            } else {
                if (col >= cw) throw_fmt(RJ_ERR_ARG, "aggregation: output attr out of range");
                const DCol& c = child.cols[col];
                if (func == RJ_AGG_KEY) {
                    if (col != n.left_attr) throw_fmt(RJ_ERR_ARG, "aggregation: RJ_AGG_KEY names another column than the key");
                    expect = kc.type;
                } else {
                    if (c.type != RJ_INT32 && c.type != RJ_INT64)
                        throw_fmt(RJ_ERR_UNSUPPORTED, "aggregation over %s column (child column %llu): INT32 and INT64 only",
                                  c.type == RJ_FP64 ? "an FP64" : "a VARCHAR", (unsigned long long)col);
                    if (func == RJ_AGG_MIN || func == RJ_AGG_MAX) expect = c.type;
                    s.need.insert((int)col);
                }
            }
            if (type != expect) throw_fmt(RJ_ERR_ARG, "aggregation: declared type differs from the function's result type");
            outs.push_back(AggOut{func, (int)col, -1});
        }
        // how the aggregated columns travel with the key
        const int KW = kc.type == RJ_INT32 ? 1 : 2;
        if (s.need.empty()) {
            s.carry_mode = CARRY_NONE;
            s.CW = 0;
        } else if (s.need.size() == 1 && !s.nullable(*s.need.begin())) {
            s.carry_mode = CARRY_COLUMN;
            s.carry_col = *s.need.begin();
            s.CW = child.cols[s.carry_col].width / 4;
            s.wide_cols = {s.carry_col};
        } else if (plan_wide_carry(s, KW, /*honour_switch=*/false)) {
            s.carry_mode = CARRY_WIDE;
        } else {
            int words = 0;
            bool any_null = false;
            for (int c : s.need) {
                words += child.cols[c].width / 4;
                any_null = any_null || s.nullable(c);
            }
            throw_fmt(RJ_ERR_UNSUPPORTED,
                      "aggregation: the aggregated columns take %d carry words; at most %d travel behind an %s key (every "
                      "distinct column its width, one more word if any is nullable, at most one 64-bit column next to "
                      "another word)",
                      words + (any_null ? 1 : 0), MAX_WORDS - KW, KW == 1 ? "INT32" : "INT64");
        }
        if (child.n == 0) return empty_rel(n, root_res);
        check_rows(child);
        for (AggOut& o : outs)
            for (size_t i = 0; i < s.wide_cols.size(); ++i)
                if (o.func >= RJ_AGG_COUNT && s.wide_cols[i] == o.col) o.slot = (int)i;

        AggParams ap{};
        ap.n_cols = (int32_t)s.wide_cols.size();
        ap.valid_word = s.valid_word;
        bool need_key = false, need_rows = false;
        {
            int word = 0;
            for (int i = 0; i < ap.n_cols; ++i) {
                const DCol& c = child.cols[s.wide_cols[i]];
                ap.col[i].word = word;
                ap.col[i].width = c.width;
                ap.col[i].valid_bit = s.valid_word >= 0 ? i : -1;
                word += c.width / 4;
            }
            for (const AggOut& o : outs) {
                need_key = need_key || o.func == RJ_AGG_KEY;
                need_rows = need_rows || o.func == RJ_AGG_COUNT_STAR;
                if (o.slot < 0) continue;
                const bool nullable = s.nullable(o.col);
                uint32_t&  need = ap.col[o.slot].need;
                if (o.func == RJ_AGG_COUNT || nullable) need |= AGG_NEED_COUNT;
                if (o.func == RJ_AGG_SUM) need |= AGG_NEED_SUM;
                if (o.func == RJ_AGG_MIN) need |= AGG_NEED_MIN;
                if (o.func == RJ_AGG_MAX) need |= AGG_NEED_MAX;
            }
        }
        prepare_wide(s);
        const TupleSrc src = make_src(JoinState(), s, JoinSpec());  // (integer keys, not pre-hashed)
        const uint32_t bits = agg_bits(child.n);
        const uint64_t cap = child.n + 1;  // every row its own group, and the NULL-key group
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] aggregation rows=%llu bits=%u cw=%d cols=%d\n", (unsigned long long)child.n, bits, s.CW,
                    ap.n_cols);

        // the node's output arrays: one row per group
        struct Arrays {
            BufP key, keyvalid, rows, nn[AGG_MAX_COLS], sum[AGG_MAX_COLS], mn[AGG_MAX_COLS], mx[AGG_MAX_COLS];
        } O, M;
        auto fill = [](AggArrays& a, const Arrays& b) {
            a.key = ptr<uint8_t>(b.key);
            a.rows = ptr<unsigned long long>(b.rows);
            for (int i = 0; i < AGG_MAX_COLS; ++i) {
                a.nn[i] = ptr<unsigned long long>(b.nn[i]);
                a.sum[i] = ptr<unsigned long long>(b.sum[i]);
                a.mn[i] = ptr<long long>(b.mn[i]);
                a.mx[i] = ptr<long long>(b.mx[i]);
            }
        };
        if (need_key) O.key = ctx->buf(cap * KW * 4);
        if (need_key && kc.valid) O.keyvalid = ctx->buf(cap);
        if (need_rows) O.rows = ctx->buf(cap * 8);
        for (int i = 0; i < ap.n_cols; ++i) {
            if (ap.col[i].need & AGG_NEED_COUNT) O.nn[i] = ctx->buf(cap * 8);
            if (ap.col[i].need & AGG_NEED_SUM) O.sum[i] = ctx->buf(cap * 8);
            if (ap.col[i].need & AGG_NEED_MIN) O.mn[i] = ctx->buf(cap * 8);
            if (ap.col[i].need & AGG_NEED_MAX) O.mx[i] = ctx->buf(cap * 8);
        }
        fill(ap.out, O);
        ap.out_keyvalid = ptr<uint8_t>(O.keyvalid);
        ap.out_cap = cap;
        ap.src = src;

        uint64_t nrows = 0;
        for (int attempt = 0;; ++attempt) {
            // [0..7] out cursor (u64), [8..11] n_heavy, [12..15] merge table overflow
            BufP counters = zeroed_counters();
            Parted P = partition(PartitionRequest::columns(src, KW, s.CW, bits));
            const uint32_t max_tasks = (uint32_t)(2 * (P.n_tuples / JN_HEAVY) + 2);
            BufP           tasks = ctx->buf((uint64_t)max_tasks * 12);
            // (one relation: a partition is "its own build side", so every partition above JN_HEAVY is cut)
            launch_heavy_tasks(L, P.off->as<uint32_t>(), P.off->as<uint32_t>(), P.NP, tasks->as<uint32_t>(),
                               counters->as<uint32_t>() + 2, max_tasks);
            // the merge table is sized from the tuples that sit in heavy partitions (an upper bound of
            // their groups), capped at first: a partition is usually heavy because its keys repeat
            uint32_t n_heavy = 0;
            read_back(&n_heavy, counters->as<uint32_t>() + 2, 4);
            n_heavy = std::min(n_heavy, max_tasks);
            uint64_t heavy_tuples = std::min<uint64_t>(P.n_tuples, (uint64_t)n_heavy * JN_HEAVY);
            if (attempt == 0) heavy_tuples = std::min<uint64_t>(heavy_tuples, 1u << 20);
            const uint32_t m_slots = n_heavy ? (1u << std::min<uint32_t>(ceil_log2(2 * heavy_tuples), 31)) : 0u;
            const uint64_t me = (uint64_t)m_slots + 2;
            M.key = ctx->buf(me * 8);
            M.rows = ctx->buf(me * 8);
            for (int i = 0; i < ap.n_cols; ++i) {
                M.nn[i] = ctx->buf(me * 8);
                M.sum[i] = ctx->buf(me * 8);
                M.mn[i] = ctx->buf(me * 8);
                M.mx[i] = ctx->buf(me * 8);
            }
            fill(ap.m, M);
            ap.m_slots = m_slots;
            ap.m_overflow = counters->as<uint32_t>() + 3;
            ap.out_cursor = counters->as<unsigned long long>();
            ap.W = P.w;
            ap.off = P.off->as<uint32_t>();
            ap.NP = P.NP;
            ap.pack = P.packed ? 1 : 0;
            ap.aos = P.aos3 ? 1 : 0;
            ap.heavy_tasks = tasks->as<uint32_t>();
            ap.n_heavy = counters->as<uint32_t>() + 2;
            ap.heavy_grid = n_heavy;
            const uint32_t mgrid = (uint32_t)std::min<uint64_t>((me + 255) / 256, (uint64_t)ctx->compute_units() * 8);
            if (O.keyvalid) RJ_HIP(hipMemsetAsync(O.keyvalid->p, 1, cap, ctx->stream));
            launch_agg_merge_init(L, ap, mgrid);
            launch_agg_parts(L, KW, s.CW, ap, n_heavy + P.NP);
            if (kc.valid) launch_agg_nullkey(L, s.CW, ap, (uint32_t)std::min<uint64_t>((child.n + JN_THREADS - 1) / JN_THREADS,
                                                                                      (uint64_t)ctx->compute_units() * 4));
            launch_agg_emit(L, KW, ap, mgrid);
            uint32_t h[4] = {0, 0, 0, 0};
            read_back(h, counters->p, 16);
            nrows = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
            if (!h[3]) break;
            // more groups in heavy partitions than the capped table holds: once more (the rounds of
            // k_agg_parts reorder a partition's memory, so from the partitioning on) with the full bound
            if (attempt == 1) throw_fmt(RJ_ERR_DEVICE, "aggregation: the merge table overflowed twice");
        }
        if (nrows > cap) throw_fmt(RJ_ERR_DEVICE, "aggregation emitted %llu rows out of %llu", (unsigned long long)nrows,
                                   (unsigned long long)cap);

        // The arrays were sized for the bound (every row its own group).  A result well below it moves
        // into arrays of its own size, so that neither this node's columns nor a parent hold on to
        // the bound's memory.
        if (nrows < cap / 2) {
            auto shrink = [&](BufP& b, uint64_t width) {
                if (!b) return;
                BufP small = ctx->buf(std::max<uint64_t>(nrows, 1) * width);
                RJ_HIP(hipMemcpyAsync(small->p, b->p, nrows * width, hipMemcpyDeviceToDevice, ctx->stream));
                b = small;
            };
            shrink(O.key, (uint64_t)KW * 4);
            shrink(O.keyvalid, 1);
            shrink(O.rows, 8);
            for (int i = 0; i < ap.n_cols; ++i) {
                shrink(O.nn[i], 8);
                shrink(O.sum[i], 8);
                shrink(O.mn[i], 8);
                shrink(O.mx[i], 8);
            }
        }

        // ---- the output columns: accumulator arrays as they are, narrowed or with validity
        Sink sink(this, root_res, nrows);
        for (size_t k = 0; k < outs.size(); ++k) {
            const AggOut& o = outs[k];
            const int32_t type = n.out_type[k];
            sink.add([&] {
                if (o.func == RJ_AGG_KEY) return dense_col(type, O.key, O.keyvalid);
                if (o.func == RJ_AGG_COUNT_STAR) return dense_col(type, O.rows);
                if (o.func == RJ_AGG_COUNT) return dense_col(type, O.nn[o.slot]);
                const BufP& acc = o.func == RJ_AGG_SUM ? O.sum[o.slot] : (o.func == RJ_AGG_MIN ? O.mn[o.slot] : O.mx[o.slot]);
                const bool  nullable = s.nullable(o.col), narrow = width_of(type) == 4;
                BufP        values = narrow ? ctx->buf(std::max<uint64_t>(nrows, 1) * 4) : acc;
                BufP        valid = nullable ? ctx->buf(std::max<uint64_t>(nrows, 1)) : BufP();
                if (narrow || nullable)
                    launch_agg_column(L, acc->as<unsigned long long>(), nullable ? O.nn[o.slot]->as<unsigned long long>() : nullptr,
                                      nrows, narrow ? 4 : 8, narrow ? values->as<uint8_t>() : nullptr, ptr<uint8_t>(valid));
                return dense_col(type, values, valid);
            }());
        }
        return sink.out;
    }

    // ---------------------------------------------------------------- selection
    // RJ_NODE_SELECT (semantics in rj.h): WHERE / HAVING / projection over the one child.  The program
    // is checked and translated into SelectProg (one ColRef per operand), k_select compacts the ids of
    // the rows it keeps, and every distinct output column is gathered through that list — at the root
    // straight into Page images.  One host sync: the row count.
    //
    // The checks of a program, in the order of the ops (the depth rules are table_from_csv's).
    static void select_program(const Rel& child, const rj_filter_op* ops, uint64_t n_ops, SelectProg& prog) {
        const size_t cw = child.cols.size();
        auto column = [&](int64_t c, const char* what) -> const DCol& {
            if (c < 0 || (uint64_t)c >= cw) throw_fmt(RJ_ERR_ARG, "select: %s out of range", what);
            const DCol& d = child.cols[(size_t)c];
            if (d.type == RJ_VARCHAR)
                throw_fmt(RJ_ERR_UNSUPPORTED, "select: predicate on a VARCHAR column (child column %lld): a VARCHAR value travels "
                                              "as a row id, its pages are not read here", (long long)c);
            return d;
        };
        int depth = 0;
        for (uint64_t k = 0; k < n_ops; ++k) {
            const rj_filter_op& o = ops[k];
            SelectOp&           d = prog.ops[k];
            d = SelectOp{};
            if (o.op == RJ_F_AND || o.op == RJ_F_OR) {
                d.kind = o.op == RJ_F_AND ? SEL_AND : SEL_OR;
                depth -= 1;
            } else if (o.op == RJ_F_NOT) {
                d.kind = SEL_NOT;
            } else if (o.op == RJ_F_HOST_BITMAP) {
                throw_fmt(RJ_ERR_ARG, "select: RJ_F_HOST_BITMAP leaf (the rows of an intermediate relation have no numbering "
                                      "a caller could see)");
            } else if (o.op == RJ_F_LIKE || o.op == RJ_F_NOT_LIKE) {
                (void)column(o.column, "predicate column");
                throw_fmt(RJ_ERR_ARG, "select: LIKE wants a VARCHAR column");
            } else if ((o.op >= RJ_F_EQ && o.op <= RJ_F_IS_NOT_NULL) || (o.op >= RJ_F_COL_EQ && o.op <= RJ_F_COL_GEQ)) {
                const DCol& a = column(o.column, "predicate column");
                d.a = a.ref();
                d.f64 = a.type == RJ_FP64;
                if (o.op == RJ_F_IS_NULL || o.op == RJ_F_IS_NOT_NULL) {
                    d.kind = o.op == RJ_F_IS_NULL ? SEL_IS_NULL : SEL_NOT_NULL;
                } else if (o.op <= RJ_F_GEQ) {
                    d.kind = SEL_LIT;
                    d.cmp = o.op - RJ_F_EQ;
                    d.literal = a.type == RJ_INT32 ? (int64_t)(int32_t)o.ivalue : o.ivalue;
                } else {
                    const DCol& b = column(o.ivalue, "right operand column");
                    if (a.type != b.type)
                        throw_fmt(RJ_ERR_ARG, "select: column comparison of different types (child columns %d and %lld)", o.column,
                                  (long long)o.ivalue);
                    d.kind = SEL_COL;
                    d.cmp = o.op - RJ_F_COL_EQ;
                    d.b = b.ref();
                }
                depth += 1;
            } else {
                throw_fmt(RJ_ERR_ARG, "select: bad filter opcode %d", o.op);
            }
            if (depth < 1 || depth > 60) throw_fmt(RJ_ERR_ARG, "select: malformed filter program");
        }
        if (n_ops && depth != 1) throw_fmt(RJ_ERR_ARG, "select: malformed filter program");
    }

    Rel select(Rel& child, const rj_node& n, Result* root_res) {
        check_projection("select", child, n);
        const uint64_t      n_ops = RJ_SELECT_N_OPS(&n);
        const rj_filter_op* ops = RJ_SELECT_OPS(&n);
        if (n_ops > (uint64_t)SEL_MAX_OPS) throw_fmt(RJ_ERR_UNSUPPORTED, "select: filter longer than %d operations", SEL_MAX_OPS);
        if (n_ops && !ops) throw_fmt(RJ_ERR_ARG, "select: %llu filter operations but a NULL program pointer", (unsigned long long)n_ops);
        std::unique_ptr<SelectProg> prog(new SelectProg());
        select_program(child, ops, n_ops, *prog);
        if (child.n == 0) return empty_rel(n, root_res);
        check_rows(child);

        // ---- the rows that pass: ids[0 .. nrows); no program = every row, and no list at all
        uint64_t nrows = child.n;
        BufP     ids;
        if (n_ops) {
            BufP dprog = ctx->buf(sizeof(SelectProg));
            ids = ctx->buf(child.n * 4);
            BufP               counters = zeroed_counters();  // [0..7] the cursor
            const uint64_t     tiles = (child.n + SEL_TILE - 1) / SEL_TILE;
            unsigned long long h = 0;
            try {
                RJ_HIP(hipMemcpyAsync(dprog->p, prog.get(), sizeof(SelectProg), hipMemcpyHostToDevice, ctx->stream));
                launch_select(L, dprog->as<SelectProg>(), (uint32_t)n_ops, (uint32_t)child.n, ids->as<uint32_t>(),
                              counters->as<unsigned long long>(),
                              (uint32_t)std::min<uint64_t>(tiles, (uint64_t)ctx->compute_units() * 8));
                read_back(&h, counters->p, 8);
            } catch (...) {
                // `prog` too is the end of a copy that may still be queued: it outlives it
                (void)hipStreamSynchronize(ctx->stream);
                throw;
            }
            nrows = h;
            if (nrows > child.n) throw_fmt(RJ_ERR_DEVICE, "select kept %llu rows out of %llu", (unsigned long long)nrows,
                                           (unsigned long long)child.n);
            if (nrows == 0) return empty_rel(n, root_res);
            if (nrows < child.n / 2) {  // (as the aggregation's arrays: nobody holds on to the bound's memory)
                BufP small = ctx->buf(nrows * 4);
                RJ_HIP(hipMemcpyAsync(small->p, ids->p, nrows * 4, hipMemcpyDeviceToDevice, ctx->stream));
                ids = small;
            }
        }
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] select rows=%llu ops=%llu kept=%llu\n", (unsigned long long)child.n, (unsigned long long)n_ops,
                    (unsigned long long)nrows);

        return emit_rows(child, n.out_idx, n.n_out, ids, ptr<uint32_t>(ids), nrows, root_res);
    }

    // a projection's outputs (select, sort): child columns under their own types
    static void check_projection(const char* what, const Rel& child, const rj_node& n) {
        for (uint64_t k = 0; k < n.n_out; ++k) {
            if (n.out_idx[k] >= child.cols.size()) throw_fmt(RJ_ERR_ARG, "%s: output attr out of range", what);
            if (child.cols[n.out_idx[k]].type != n.out_type[k])
                throw_fmt(RJ_ERR_ARG, "%s: declared type differs from the child column's type", what);
        }
    }

    // The tail of a selection and of a sort, and the passed-through columns of a window and a map node:
    // columns cols[0 .. n_cols) of `child` go to `sink`, output row i being row idx[i] (sink.out.n of
    // them; idx points into `ids`, in this order; nullptr = the child's own rows, all of them).  Every
    // distinct column is gathered once — at the root straight into Page images.
    void emit_rows(const Rel& child, const uint64_t* cols, uint64_t n_cols, const BufP& ids, const uint32_t* idx, Sink& sink) {
        const uint64_t nrows = sink.out.n;
        for (uint64_t k = 0; k < n_cols; ++k) {
            const DCol& src = child.cols[cols[k]];
            sink.add(cols[k], [&] {
                if (!idx) return src;  // (without a list the column itself)
                if (src.kind == COL_IOTA) {  // row ids of the base table ARE the list
                    DCol d = dense_like(src, ids);
                    d.ptr = reinterpret_cast<const uint8_t*>(idx);  // (`idx` itself may start inside `ids`)
                    return d;
                }
                // a root column without NULLs goes straight into its Page images
                const bool to_pages = sink.res && src.type != RJ_VARCHAR && src.valid == nullptr;
                const int  mode = to_pages ? (src.width == 4 ? ST_PAGED32 : ST_PAGED64) : (src.width == 4 ? ST_DENSE32 : ST_DENSE64);
                BufP       values = ctx->buf(stream_bytes(mode, nrows));
                DCol       d = dense_like(src, values, src.valid ? ctx->buf(nrows) : BufP());
                if (to_pages) d.kind = COL_PAGED;
                launch_gather(L, src.ref(), idx, nrows, OutStream{values->as<uint8_t>(), mode, 0}, ptr<uint8_t>(d.hold_valid));
                if (to_pages) launch_finish_pages(L, values->as<uint8_t>(), nrows, src.width);
                return d;
            });
        }
    }
    Rel emit_rows(const Rel& child, const uint64_t* cols, uint64_t n_cols, const BufP& ids, const uint32_t* idx, uint64_t nrows,
                  Result* root_res) {
        Sink sink(this, root_res, nrows);
        emit_rows(child, cols, n_cols, ids, idx, sink);
        return sink.out;
    }

    // ---------------------------------------------------------------------- sort
    // RJ_NODE_SORT (semantics in rj.h): ORDER BY / LIMIT / OFFSET over the one child.  A stable LSD radix
    // sort of {encoded key, row id}: the key columns from the last to the first, each encoded through
    // the permutation the columns behind it left (sort_column), so that stability gives the
    // lexicographic order.  Only the rows of the slice are gathered afterwards (emit_rows).  One host
    // sync per key column: its digit histograms, which say what passes it needs.
    //
    // One key column: `perm` (n ids, or none = the child's own order) -> the order with this column as
    // the most significant key.  A pass whose digit has ONE non-empty bin over all rows is not
    // launched; a column without any pass leaves `perm` as it is.
    void sort_column(const DCol& c, int32_t flags, uint32_t n, BufP& perm) {
        const int      W = c.width;
        const uint32_t n_tiles = n / SORT_TILE + (n % SORT_TILE != 0);
        BufP           keys = ctx->buf((uint64_t)n * W);
        BufP           hist = ctx->buf(SORT_HIST_WORDS * 4);
        std::vector<uint32_t> h(SORT_HIST_WORDS);
        RJ_HIP(hipMemsetAsync(hist->p, 0, SORT_HIST_WORDS * 4, ctx->stream));
        const uint32_t chunks = n / SORT_THREADS + (n % SORT_THREADS != 0);
        launch_sort_encode(L, c.ref(), ptr<uint32_t>(perm), n, c.type == RJ_FP64, flags, keys->as<uint8_t>(), hist->as<uint32_t>(),
                           std::min<uint32_t>(chunks, (uint32_t)ctx->compute_units() * 8));
        read_back(h.data(), hist->p, SORT_HIST_WORDS * 4);
        std::vector<int> passes;  // digit positions with more than one non-empty bin, the NULL digit last
        for (int p = 0; p <= SORT_NULL_DIGIT; ++p) {
            if (p >= W && p != SORT_NULL_DIGIT) continue;
            int bins = 0;
            for (int b = 0; b < SORT_RADIX; ++b) bins += h[(size_t)p * SORT_RADIX + b] != 0;
            if (bins > 1) passes.push_back(p);
        }
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] sort column rows=%u width=%d flags=%d passes=%zu\n", n, W, flags, passes.size());
        if (passes.empty()) return;
        BufP table = ctx->buf((uint64_t)SORT_RADIX * n_tiles * 4);
        BufP keys2, ids_in = perm, spare;  // (ids_in: none = positions)
        for (size_t q = 0; q < passes.size(); ++q) {
            const int  p = passes[q];
            const bool flag = p == SORT_NULL_DIGIT;
            // the keys travel only as far as a later pass reads them
            const bool keys_on = !flag && q + 1 < passes.size() && passes[q + 1] != SORT_NULL_DIGIT;
            if (keys_on && !keys2) keys2 = ctx->buf((uint64_t)n * W);
            BufP           ids_out = spare ? spare : ctx->buf((uint64_t)n * 4);
            const int      mode = flag ? SORT_FLAG : (W == 4 ? SORT_KEY32 : SORT_KEY64);
            const uint32_t null_digit = (flags & RJ_SORT_NULLS_FIRST) ? 0u : 1u, shift = flag ? 0u : 8u * (uint32_t)p;
            const uint32_t* in = ptr<uint32_t>(ids_in);
            launch_sort_count(L, mode, keys->as<uint8_t>(), in, c.valid, null_digit, n, shift, table->as<uint32_t>());
            launch_sort_scan(L, hist->as<uint32_t>() + (size_t)p * SORT_RADIX, n, table->as<uint32_t>());
            launch_sort_scatter(L, mode, keys->as<uint8_t>(), in, c.valid, null_digit, n, shift, table->as<uint32_t>(),
                                keys_on ? keys2->as<uint8_t>() : nullptr, ids_out->as<uint32_t>());
            spare = ids_in;
            ids_in = ids_out;
            if (keys_on) std::swap(keys, keys2);
        }
        perm = ids_in;
    }

    // The key list of a sort, a grouping or a window node (`what`), checked in the order of the keys
    // before the child's rows are looked at.
    static std::vector<rj_sort_key> checked_keys(const char* what, const Rel& child, const rj_sort_key* keys, uint64_t n_keys) {
        if (n_keys > (uint64_t)SORT_MAX_KEYS) throw_fmt(RJ_ERR_UNSUPPORTED, "%s: more than %d keys", what, SORT_MAX_KEYS);
        if (n_keys && !keys) throw_fmt(RJ_ERR_ARG, "%s: %llu keys but a NULL key pointer", what, (unsigned long long)n_keys);
        for (uint64_t k = 0; k < n_keys; ++k) {
            if (keys[k].column < 0 || (uint64_t)keys[k].column >= child.cols.size())
                throw_fmt(RJ_ERR_ARG, "%s: key column out of range", what);
            if (keys[k].flags & ~(RJ_SORT_DESC | RJ_SORT_NULLS_FIRST)) throw_fmt(RJ_ERR_ARG, "%s: unknown key flags %d", what, keys[k].flags);
            if (child.cols[(size_t)keys[k].column].type == RJ_VARCHAR)
                throw_fmt(RJ_ERR_UNSUPPORTED, "%s: VARCHAR key (child column %d): a VARCHAR value travels as a row id, its pages "
                                              "are not read here", what, keys[k].column);
        }
        return std::vector<rj_sort_key>(keys, keys + n_keys);
    }
    // The rows of `child` in the order of the keys: the permutation, or none where no pass moved a row.
    // The last key first; a key behind an earlier one on the same column is skipped: nothing is left
    // to order there, rows that tie on the column tie again.
    BufP order_by(const Rel& child, const std::vector<rj_sort_key>& keys) {
        BufP perm;
        for (size_t k = keys.size(); k-- > 0;) {
            bool shadowed = false;
            for (size_t j = 0; j < k; ++j) shadowed = shadowed || keys[j].column == keys[k].column;
            if (!shadowed) sort_column(child.cols[(size_t)keys[k].column], keys[k].flags, (uint32_t)child.n, perm);
        }
        return perm;
    }

    Rel sort(Rel& child, const rj_node& n, Result* root_res, bool ordered = false) {
        check_projection("sort", child, n);
        const uint64_t limit = RJ_SORT_LIMIT(&n), offset = RJ_SORT_OFFSET(&n);
        const std::vector<rj_sort_key> keys = checked_keys("sort", child, RJ_SORT_KEYS(&n), RJ_SORT_N_KEYS(&n));
        if (child.n == 0) return empty_rel(n, root_res);
        check_rows(child);
        // the slice [begin, begin + count): offset + limit is never formed
        const uint64_t begin = std::min<uint64_t>(offset, child.n), count = std::min<uint64_t>(limit, child.n - begin);
        if (count == 0) return empty_rel(n, root_res);
        const bool whole = count == child.n;
        // below another node the order is nobody's business: without a slice the child passes through
        // (not below the MAPs of a root, which keep the order: `ordered`)
        BufP perm;
        if (root_res || ordered || !whole) perm = order_by(child, keys);
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] sort rows=%llu keys=%llu begin=%llu count=%llu permuted=%d\n", (unsigned long long)child.n,
                    (unsigned long long)keys.size(), (unsigned long long)begin, (unsigned long long)count, perm ? 1 : 0);
        const uint32_t* idx = perm ? perm->as<uint32_t>() + begin : nullptr;
        if (!perm && !whole) {  // no pass moved a row: the slice is a run of positions
            perm = ctx->buf(count * 4);
            idx = perm->as<uint32_t>();
            launch_sort_iota(L, perm->as<uint32_t>(), (uint32_t)begin, (uint32_t)count);
        }
        return emit_rows(child, n.out_idx, n.n_out, perm, idx, count, root_res);
    }

    // -------------------------------------------------------------------- grouping
    // RJ_NODE_GROUP (semantics in rj.h): GROUP BY any number of INT32 / INT64 / FP64 keys, or none.  The
    // rows are ordered by the keys as a sort orders them (sort_column, the last key first), which puts
    // every group into one run of the permutation; k_group_heads marks where the runs begin, a scan
    // numbers them, and k_group_reduce reduces one aggregated column per launch, run by run
    // (rj_group.hip).  Host syncs: one per key column (its digit histograms) and one for the group
    // count, which sizes the outputs.  Nothing is sized for a bound, nothing is attempted twice.
    struct GroupCol {
        bool want_nn = false, want_sum = false, want_mn = false, want_mx = false, want_fsum = false;
        BufP nn, sum, mn, mx, fsum;
    };
    Rel group(Rel& child, const rj_node& n, Result* root_res) {
        const size_t                   cw = child.cols.size();
        const std::vector<rj_sort_key> keys = checked_keys("group", child, RJ_GROUP_KEYS(&n), RJ_GROUP_N_KEYS(&n));
        const uint64_t                 n_keys = keys.size();
        std::vector<int>               key_cols;  // the distinct key columns, the first key's first
        for (const rj_sort_key& key : keys)
            if (std::find(key_cols.begin(), key_cols.end(), key.column) == key_cols.end()) key_cols.push_back(key.column);
        struct Out {
            uint32_t func;
            int      col;
        };
        std::vector<Out>        outs;
        std::map<int, GroupCol> agg;  // per distinct aggregated column
        bool                    want_rows = false;
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint32_t func = RJ_AGG_FUNC(n.out_idx[k]);
            const uint64_t col = RJ_AGG_COL(n.out_idx[k]);
            if (func > RJ_AGG_MAX && func != RJ_AGG_FSUM) throw_fmt(RJ_ERR_ARG, "group: unknown function code %u", func);
            int32_t expect = RJ_INT64;
            if (func == RJ_AGG_COUNT_STAR) {
                if (col != 0) throw_fmt(RJ_ERR_ARG, "group: COUNT(*) takes no column");
                want_rows = true;
            } else {
                if (col >= cw) throw_fmt(RJ_ERR_ARG, "group: output attr out of range");
                const DCol& c = child.cols[col];
                if (func == RJ_AGG_KEY) {
                    if (std::find(key_cols.begin(), key_cols.end(), (int)col) == key_cols.end())
                        throw_fmt(RJ_ERR_ARG, "group: RJ_AGG_KEY names child column %llu, which is not a key", (unsigned long long)col);
                    expect = c.type;
                } else {
                    if (c.type == RJ_VARCHAR)
                        throw_fmt(RJ_ERR_UNSUPPORTED, "group: aggregate over a VARCHAR column (child column %llu): a VARCHAR value "
                                                      "travels as a row id, its pages are not read here", (unsigned long long)col);
                    if (func == RJ_AGG_SUM && c.type == RJ_FP64)
                        throw_fmt(RJ_ERR_UNSUPPORTED, "group: SUM over an FP64 column (child column %llu): a floating-point sum depends "
                                                      "on the order of the rows; RJ_AGG_FSUM is the exactly rounded FP64 sum",
                                  (unsigned long long)col);
                    if (func == RJ_AGG_FSUM && c.type != RJ_FP64)
                        throw_fmt(RJ_ERR_ARG, "group: FSUM takes an FP64 column (child column %llu is not one): RJ_AGG_SUM is the "
                                              "integer sum", (unsigned long long)col);
                    if (func == RJ_AGG_MIN || func == RJ_AGG_MAX) expect = c.type;
                    if (func == RJ_AGG_FSUM) expect = RJ_FP64;
                    GroupCol& g = agg[(int)col];
                    g.want_nn = true;  // (COUNT itself, and what says whether SUM / MIN / MAX are NULL)
                    g.want_sum = g.want_sum || func == RJ_AGG_SUM;
                    g.want_mn = g.want_mn || func == RJ_AGG_MIN;
                    g.want_mx = g.want_mx || func == RJ_AGG_MAX;
                    g.want_fsum = g.want_fsum || func == RJ_AGG_FSUM;
                }
            }
            if (n.out_type[k] != expect) throw_fmt(RJ_ERR_ARG, "group: declared type differs from the function's result type");
            outs.push_back(Out{func, (int)col});
        }
        check_rows(child);
        if (child.n == 0 && n_keys) return empty_rel(n, root_res);
        const uint32_t rows = (uint32_t)child.n;

        // ---- the order, the heads, the group count
        BufP     perm, masks, tile_base;
        uint32_t G = 1;
        if (n_keys) {
            perm = order_by(child, keys);
            const uint32_t n_tiles = rows / GROUP_TILE + (rows % GROUP_TILE != 0);
            masks = ctx->buf(((uint64_t)rows + 63) / 64 * 8);
            tile_base = ctx->buf(((uint64_t)n_tiles + 1) * 4);
            BufP tile_heads = ctx->buf((uint64_t)n_tiles * 4), total = ctx->buf(4);
            for (size_t k = 0; k < key_cols.size(); ++k) {
                const DCol& c = child.cols[(size_t)key_cols[k]];
                launch_group_heads(L, c.ref(), ptr<uint32_t>(perm), rows, c.type == RJ_FP64, k == 0, k + 1 == key_cols.size(),
                                   masks->as<unsigned long long>(), tile_heads->as<uint32_t>());
            }
            launch_group_scan(L, tile_heads->as<uint32_t>(), rows, tile_base->as<uint32_t>(), total->as<uint32_t>());
            read_back(&G, total->p, 4);
            if (G == 0 || G > rows) throw_fmt(RJ_ERR_DEVICE, "group: %u groups out of %u rows", G, rows);
        }
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] group rows=%u keys=%llu groups=%u permuted=%d columns=%zu\n", rows, (unsigned long long)n_keys, G,
                    perm ? 1 : 0, agg.size());
        const uint32_t*           dperm = ptr<uint32_t>(perm);
        const unsigned long long* dmasks = ptr<unsigned long long>(masks);
        const uint32_t*           dbase = ptr<uint32_t>(tile_base);

        // ---- the keys that are output: one array per distinct column
        std::map<int, DCol> key_out;
        for (const Out& o : outs) {
            if (o.func != RJ_AGG_KEY || key_out.count(o.col)) continue;
            const DCol& c = child.cols[(size_t)o.col];
            const DCol  d = new_col(c.type, G, c.valid != nullptr);
            launch_group_keys(L, c.ref(), dperm, rows, c.type == RJ_FP64, dmasks, dbase, G, d.hold->as<uint8_t>(),
                              ptr<uint8_t>(d.hold_valid));
            key_out[o.col] = d;
        }

        // ---- the reductions: one launch per distinct aggregated column, the first of which counts the rows too
        const uint32_t max_grid = ctx->tune.group_grid > 0 ? (uint32_t)ctx->tune.group_grid : (uint32_t)ctx->compute_units() * 8u;
        BufP           rows_acc = want_rows ? ctx->buf((uint64_t)G * 8) : BufP();
        bool           rows_done = !want_rows;
        using ull = unsigned long long;
        for (auto& kv : agg) {
            const DCol& c = child.cols[(size_t)kv.first];
            GroupCol&   g = kv.second;
            if (g.want_nn) g.nn = ctx->buf((uint64_t)G * 8);
            if (g.want_sum) g.sum = ctx->buf((uint64_t)G * 8);
            if (g.want_mn) g.mn = ctx->buf((uint64_t)G * 8);
            if (g.want_mx) g.mx = ctx->buf((uint64_t)G * 8);
            const GroupAcc acc{rows_done ? nullptr : ptr<ull>(rows_acc), ptr<ull>(g.nn), ptr<ull>(g.sum), ptr<ull>(g.mn), ptr<ull>(g.mx)};
            const ColRef   ref = c.ref();
            launch_group_reduce(L, &ref, dperm, rows, c.type == RJ_FP64, dmasks, dbase, G, acc, max_grid);
            rows_done = true;
            if (g.want_fsum) {  // (the count above says which of its sums are NULL)
                g.fsum = ctx->buf((uint64_t)G * 8);
                BufP scratch = ctx->buf(fsum_scratch_bytes(rows, max_grid));
                if (ctx->tune.diag >= 2) fprintf(stderr, "[rj diag] group fsum column=%d rows=%u groups=%u\n", kv.first, rows, G);
                launch_fsum(L, ref, dperm, rows, dmasks, dbase, G, g.fsum->as<ull>(), max_grid, scratch->as<uint8_t>());
            }
        }
        if (!rows_done) {
            const GroupAcc acc{ptr<ull>(rows_acc), nullptr, nullptr, nullptr, nullptr};
            launch_group_reduce(L, nullptr, dperm, rows, false, dmasks, dbase, G, acc, max_grid);
        }

        // ---- the output columns
        Sink sink(this, root_res, G);
        for (size_t k = 0; k < outs.size(); ++k) {
            const Out&    o = outs[k];
            const int32_t type = n.out_type[k];
            sink.add([&] {
                if (o.func == RJ_AGG_KEY) return key_out.at(o.col);
                if (o.func == RJ_AGG_COUNT_STAR) return dense_col(type, rows_acc);
                if (o.func == RJ_AGG_COUNT) return dense_col(type, agg.at(o.col).nn);
                const GroupCol& g = agg.at(o.col);
                const DCol&     c = child.cols[(size_t)o.col];
                const BufP&     acc = o.func == RJ_AGG_FSUM ? g.fsum : (o.func == RJ_AGG_SUM ? g.sum : (o.func == RJ_AGG_MIN ? g.mn : g.mx));
                // NULL where the group has no non-NULL value: a nullable column, or the one row over no rows
                const bool nullable = c.valid != nullptr || rows == 0;
                const int  decode = o.func == RJ_AGG_SUM || o.func == RJ_AGG_FSUM ? GROUP_RAW : (c.type == RJ_FP64 ? GROUP_KEYF64 : (c.type == RJ_INT32 ? GROUP_KEY32 : GROUP_KEY64));
                if (decode == GROUP_RAW && !nullable) return dense_col(type, acc);
                const DCol d = new_col(type, G, nullable);
                launch_group_column(L, acc->as<ull>(), nullable ? g.nn->as<ull>() : nullptr, G, decode, d.width, d.hold->as<uint8_t>(),
                                    ptr<uint8_t>(d.hold_valid));
                return d;
            }());
        }
        return sink.out;
    }

    // ------------------------------------------------------------------ set operations
    // RJ_NODE_SETOP (semantics in rj.h): UNION / INTERSECT / EXCEPT [ALL] of the two children.  UNION ALL
    // puts every distinct pair of columns one behind the other (k_setop_concat) and is done.  The five
    // other operations do that into a relation U of l.n + r.n rows (row id < l.n: a left row), order U by
    // every column as a sort does and cut it into runs of equal rows as a grouping does; the k_setop_*
    // kernels (rj_setop.hip) then count every run's rows and left rows, turn them into the run's
    // multiplicity, scan the multiplicities and list, per output row, the run it is a copy of; the runs'
    // canonical values (k_group_keys) are gathered through that list.  UNION takes every run once: the
    // canonical values are the result.  Host syncs: one per column (its digit histograms), one for
    // the run count and one for the output's row count.
    static_assert((int)SETOP_UNION_ALL == (int)RJ_SET_UNION_ALL && (int)SETOP_UNION == (int)RJ_SET_UNION &&
                      (int)SETOP_INTERSECT == (int)RJ_SET_INTERSECT && (int)SETOP_INTERSECT_ALL == (int)RJ_SET_INTERSECT_ALL &&
                      (int)SETOP_EXCEPT == (int)RJ_SET_EXCEPT && (int)SETOP_EXCEPT_ALL == (int)RJ_SET_EXCEPT_ALL,
                  "SetOp mirrors rj_setop");
    Rel setop(Rel& l, Rel& r, const rj_node& n, Result* root_res) {
        const uint64_t op = RJ_SETOP_OP(&n);
        if (op > RJ_SET_EXCEPT_ALL) throw_fmt(RJ_ERR_ARG, "setop: unknown operation code %llu", (unsigned long long)op);
        if (n.n_out == 0) throw_fmt(RJ_ERR_ARG, "setop: no output columns");
        const bool sorting = op != RJ_SET_UNION_ALL;
        std::vector<uint64_t> pairs;       // the distinct pairs, the first output's first
        std::vector<uint64_t> out_cols;    // per output: its pair's index
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint32_t lc = RJ_SETOP_LCOL(n.out_idx[k]), rc = RJ_SETOP_RCOL(n.out_idx[k]);
            if (lc >= l.cols.size()) throw_fmt(RJ_ERR_ARG, "setop: left column %u out of range", lc);
            if (rc >= r.cols.size()) throw_fmt(RJ_ERR_ARG, "setop: right column %u out of range", rc);
            if (l.cols[lc].type != r.cols[rc].type)
                throw_fmt(RJ_ERR_ARG, "setop: left column %u and right column %u differ in type (no implicit cast: map below)", lc, rc);
            if (l.cols[lc].type != n.out_type[k]) throw_fmt(RJ_ERR_ARG, "setop: declared type differs from the paired columns' type");
            const auto it = std::find(pairs.begin(), pairs.end(), n.out_idx[k]);
            out_cols.push_back((uint64_t)(it - pairs.begin()));
            if (it == pairs.end()) pairs.push_back(n.out_idx[k]);
        }
        if (sorting && pairs.size() > (size_t)SORT_MAX_KEYS)
            throw_fmt(RJ_ERR_UNSUPPORTED, "setop: more than %d distinct column pairs in a sorting operation", SORT_MAX_KEYS);
        for (uint64_t p : pairs) {
            const DCol &a = l.cols[RJ_SETOP_LCOL(p)], &b = r.cols[RJ_SETOP_RCOL(p)];
            if (a.type != RJ_VARCHAR) continue;
            if (sorting)
                throw_fmt(RJ_ERR_UNSUPPORTED, "setop: VARCHAR pair (left column %u) in a sorting operation: a VARCHAR value travels as a "
                                              "row id, its pages are not read here", RJ_SETOP_LCOL(p));
            // (a relation without rows that no scan made — an empty selection's, say — has forgotten where its
            // row ids would point: it holds none, so there is nothing to disagree about)
            const bool known = !(l.n == 0 && a.vc_table < 0) && !(r.n == 0 && b.vc_table < 0);
            if (known && (a.vc_table != b.vc_table || a.vc_col != b.vc_col))
                throw_fmt(RJ_ERR_UNSUPPORTED, "setop: VARCHAR pair (left column %u, right column %u) from two base-table columns: one "
                                              "row-id column cannot point into two tables", RJ_SETOP_LCOL(p), RJ_SETOP_RCOL(p));
        }
        const uint64_t rows64 = l.n + r.n;
        if (l.n > 0xfffffff0ull || r.n > 0xfffffff0ull || rows64 > 0xfffffff0ull)
            throw_fmt(RJ_ERR_UNSUPPORTED, "setop: more than 2^32 - 16 rows in the two children together");
        if (rows64 == 0) return empty_rel(n, root_res);
        const uint32_t rows = (uint32_t)rows64, n_left = (uint32_t)l.n;
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] setop op=%llu left=%llu right=%llu pairs=%zu\n", (unsigned long long)op, (unsigned long long)l.n,
                    (unsigned long long)r.n, pairs.size());

        // one column of both children; to_pages: straight into Page images (a root column without NULLs)
        auto concat = [&](uint64_t p, bool to_pages) {
            const DCol &a = l.cols[RJ_SETOP_LCOL(p)], &b = r.cols[RJ_SETOP_RCOL(p)];
            const bool nullable = a.valid != nullptr || b.valid != nullptr;
            const int  mode = to_pages ? (a.width == 4 ? ST_PAGED32 : ST_PAGED64) : (a.width == 4 ? ST_DENSE32 : ST_DENSE64);
            BufP       values = ctx->buf(stream_bytes(mode, rows));
            DCol       d = dense_like(a, values, nullable ? ctx->buf(rows) : BufP());
            if (to_pages) d.kind = COL_PAGED;
            launch_setop_concat(L, a.ref(), b.ref(), n_left, rows, OutStream{values->as<uint8_t>(), mode, 0}, ptr<uint8_t>(d.hold_valid));
            if (to_pages) launch_finish_pages(L, values->as<uint8_t>(), rows, a.width);
            return d;
        };

        if (!sorting) {
            Sink sink(this, root_res, rows);
            for (uint64_t k = 0; k < n.n_out; ++k) {
                const uint64_t p = n.out_idx[k];
                sink.add(p, [&] {
                    // one child without rows: the other child's column as it is
                    if (r.n == 0) return l.cols[RJ_SETOP_LCOL(p)];
                    if (l.n == 0) return r.cols[RJ_SETOP_RCOL(p)];
                    const DCol &a = l.cols[RJ_SETOP_LCOL(p)], &b = r.cols[RJ_SETOP_RCOL(p)];
                    return concat(p, root_res && a.type != RJ_VARCHAR && !a.valid && !b.valid);
                });
            }
            return sink.out;
        }

        // ---- U, its order, the heads, the run count
        Rel U;
        U.n = rows;
        std::vector<rj_sort_key> keys;
        for (size_t c = 0; c < pairs.size(); ++c) {
            U.cols.push_back(concat(pairs[c], false));
            keys.push_back(rj_sort_key{(int32_t)c, 0});
        }
        const BufP     perm = order_by(U, keys);
        const uint32_t n_tiles = rows / GROUP_TILE + (rows % GROUP_TILE != 0);
        BufP           masks = ctx->buf(((uint64_t)rows + 63) / 64 * 8), tile_base = ctx->buf(((uint64_t)n_tiles + 1) * 4);
        BufP           tile_heads = ctx->buf((uint64_t)n_tiles * 4), total = ctx->buf(4);
        for (size_t c = 0; c < U.cols.size(); ++c) {
            const DCol& col = U.cols[c];
            launch_group_heads(L, col.ref(), ptr<uint32_t>(perm), rows, col.type == RJ_FP64, c == 0, c + 1 == U.cols.size(),
                               masks->as<unsigned long long>(), tile_heads->as<uint32_t>());
        }
        launch_group_scan(L, tile_heads->as<uint32_t>(), rows, tile_base->as<uint32_t>(), total->as<uint32_t>());
        uint32_t G = 0;
        read_back(&G, total->p, 4);
        if (G == 0 || G > rows) throw_fmt(RJ_ERR_DEVICE, "setop: %u runs out of %u rows", G, rows);

        // ---- the runs' rows and left rows -> multiplicities -> where every run's copies go
        const uint32_t max_grid = ctx->tune.setop_grid > 0 ? (uint32_t)ctx->tune.setop_grid : (uint32_t)ctx->compute_units() * 8u;
        uint32_t       n_result = G;  // (UNION: every run once)
        BufP           run_of;
        if (op != RJ_SET_UNION) {
            BufP            tile_left = ctx->buf((uint64_t)n_tiles * 4), tile_lbase = ctx->buf(((uint64_t)n_tiles + 1) * 4);
            BufP            start = ctx->buf(((uint64_t)G + 1) * 4), left = ctx->buf(((uint64_t)G + 1) * 4);
            const SetopRuns runs{start->as<uint32_t>(), left->as<uint32_t>()};
            launch_setop_runs(L, ptr<uint32_t>(perm), rows, n_left, masks->as<unsigned long long>(), tile_base->as<uint32_t>(), G,
                              tile_left->as<uint32_t>(), tile_lbase->as<uint32_t>(), runs, max_grid);
            const uint32_t r_tiles = G / SETOP_TILE + (G % SETOP_TILE != 0);
            BufP           tile_m = ctx->buf((uint64_t)r_tiles * 4), tile_mbase = ctx->buf(((uint64_t)r_tiles + 1) * 4);
            BufP           off = ctx->buf(((uint64_t)G + 1) * 4), n_out_dev = ctx->buf(4);
            launch_setop_offsets(L, runs, G, (int)op, tile_m->as<uint32_t>(), tile_mbase->as<uint32_t>(), off->as<uint32_t>(),
                                 n_out_dev->as<uint32_t>(), max_grid);
            read_back(&n_result, n_out_dev->p, 4);
            if (n_result > rows) throw_fmt(RJ_ERR_DEVICE, "setop: %u result rows out of %u rows", n_result, rows);
            if (n_result == 0) return empty_rel(n, root_res);
            run_of = ctx->buf((uint64_t)n_result * 4);
            launch_setop_emit(L, off->as<uint32_t>(), G, n_result, run_of->as<uint32_t>(), max_grid);
        }
        if (ctx->tune.diag >= 2) fprintf(stderr, "[rj diag] setop rows=%u runs=%u result=%u permuted=%d\n", rows, G, n_result, perm ? 1 : 0);

        // ---- the runs' canonical values, gathered through the list (the run order is the result's order)
        Rel K;
        K.n = G;
        for (const DCol& col : U.cols) {
            const DCol d = new_col(col.type, G, col.valid != nullptr);
            launch_group_keys(L, col.ref(), ptr<uint32_t>(perm), rows, col.type == RJ_FP64, masks->as<unsigned long long>(),
                              tile_base->as<uint32_t>(), G, d.hold->as<uint8_t>(), ptr<uint8_t>(d.hold_valid));
            K.cols.push_back(d);
        }
        return emit_rows(K, out_cols.data(), out_cols.size(), run_of, ptr<uint32_t>(run_of), n_result, root_res);
    }

    // ---------------------------------------------------------------------- window
    // RJ_NODE_WINDOW (semantics in rj.h): ROW_NUMBER / RANK / DENSE_RANK and COUNT / SUM / MIN / MAX OVER
    // (PARTITION BY ... ORDER BY ...).  The rows are ordered by (partition keys, order keys) as a sort
    // orders them (sort_column, the last key first); k_group_heads marks where the partitions begin (P)
    // and, OR-ed over the order keys into a copy of P, where the peer groups begin (Q); the k_win_*
    // kernels (rj_window.hip) turn the two masks into the ranks and every row's peer end, and scan one
    // value column per set of launches.  The passed-through columns are gathered through the permutation
    // as a sort's (emit_rows).  Host syncs: those of sort_column only — the result has the child's rows.
    // The functions from RJ_WIN_LAG on (ROWS frames, LAG / LEAD / FIRST_VALUE / LAST_VALUE, NTILE) sit on top:
    // a second k_win_ranks launch with Q := P gives every position its partition, and the k_frame_* kernels
    // (rj_frame.hip) pick a row, subtract two entries of the scan or walk a range-extreme tree per frame
    // (frame_column).  A plan without such a function launches and allocates what it did without them.
    struct WinCol {
        bool want_sum = false, want_mn = false, want_mx = false;
        bool want_tree_mn = false, want_tree_mx = false;  // ROWS_MIN / ROWS_MAX: the range-extreme trees (rj_frame.hip)
        BufP nn, sum, mn, mx, tree_mn, tree_mx;
    };
    // One result column of a function from RJ_WIN_LAG on (the k_frame_* kernels, rj_frame.hip) over the
    // frame [lo, hi]; `w`: the scans and trees of the value column, for the ROWS aggregates.
    DCol frame_column(const Rel& child, uint32_t func, int col, int64_t lo, int64_t hi, int32_t type, uint32_t rows, const uint32_t* dperm,
                      const FrameRows& fr, const WinCol* w) {
        using ull = unsigned long long;
        if (func == RJ_WIN_NTILE) {
            const DCol d = new_col(type, rows, false);
            launch_frame_ntile(L, rows, fr, lo, d.hold->as<ull>());
            return d;
        }
        if (func == RJ_WIN_ROWS_COUNT_STAR) {
            const DCol d = new_col(type, rows, false);
            launch_frame_sum(L, nullptr, nullptr, rows, fr, lo, hi, FRAME_COUNT_STAR, d.hold->as<ull>(), nullptr);
            return d;
        }
        const DCol& c = child.cols[(size_t)col];
        if (func <= RJ_WIN_LAST_VALUE) {  // LAG, LEAD, FIRST_VALUE, LAST_VALUE: always nullable
            const DCol d = new_col(type, rows, true);
            launch_frame_pick(L, c.ref(), dperm, rows, fr, lo, hi, func == RJ_WIN_LAST_VALUE ? FRAME_LAST : FRAME_FIRST, d.hold->as<uint8_t>(),
                              d.hold_valid->as<uint8_t>());
            return d;
        }
        if (func == RJ_WIN_ROWS_COUNT) {
            const DCol d = new_col(type, rows, false);
            launch_frame_sum(L, ptr<uint32_t>(w->nn), nullptr, rows, fr, lo, hi, FRAME_COUNT, d.hold->as<ull>(), nullptr);
            return d;
        }
        // NULL where the frame has no non-NULL value: a nullable column's frames can, and a frame that can miss the current row
        const DCol d = new_col(type, rows, c.valid != nullptr || lo > 0 || hi < 0);
        if (func == RJ_WIN_ROWS_SUM) {
            launch_frame_sum(L, ptr<uint32_t>(w->nn), ptr<ull>(w->sum), rows, fr, lo, hi, FRAME_SUM, d.hold->as<ull>(), ptr<uint8_t>(d.hold_valid));
        } else {
            const bool is_max = func == RJ_WIN_ROWS_MAX;
            const int  decode = c.type == RJ_FP64 ? GROUP_KEYF64 : (c.type == RJ_INT32 ? GROUP_KEY32 : GROUP_KEY64);
            launch_frame_extreme(L, ptr<ull>(is_max ? w->tree_mx : w->tree_mn), ptr<uint32_t>(w->nn), rows, fr, lo, hi, is_max, decode, d.width,
                                 d.hold->as<uint8_t>(), ptr<uint8_t>(d.hold_valid));
        }
        return d;
    }

    Rel window(Rel& child, const rj_node& n, Result* root_res) {
        const size_t   cw = child.cols.size();
        const uint64_t n_keys = RJ_WINDOW_N_KEYS(&n), n_part = RJ_WINDOW_N_PART(&n);
        // (behind the limit of the key count, ahead of the other checks of the list)
        if (n_keys <= (uint64_t)SORT_MAX_KEYS && n_part > n_keys)
            throw_fmt(RJ_ERR_ARG, "window: %llu partition keys out of %llu keys", (unsigned long long)n_part, (unsigned long long)n_keys);
        const std::vector<rj_sort_key> keys = checked_keys("window", child, RJ_WINDOW_KEYS(&n), n_keys);
        std::vector<int> part_cols, order_cols;  // the distinct key columns; an order key that is a partition key too orders nothing
        for (uint64_t k = 0; k < n_keys; ++k) {
            const bool in_part = std::find(part_cols.begin(), part_cols.end(), keys[k].column) != part_cols.end();
            if (k < n_part) {
                if (!in_part) part_cols.push_back(keys[k].column);
            } else if (!in_part && std::find(order_cols.begin(), order_cols.end(), keys[k].column) == order_cols.end()) {
                order_cols.push_back(keys[k].column);
            }
        }
        struct Out {
            uint32_t func;
            int      col;
            int64_t  lo, hi;  // from RJ_WIN_LAG on: the frame (LAG / LEAD k as the frame [-k, -k] / [k, k]); NTILE: lo = n
        };
        std::vector<Out>      outs;
        std::map<int, WinCol> agg;  // per distinct value column
        bool                  want[RJ_WIN_COUNT_STAR + 1] = {false, false, false, false, false};
        bool                  any_frame = false;  // a function that needs every position's partition
        bool                  any_peer = false;   // ... every position's peer end: an aggregate under the default frame
        const rj_win_arg*     args = nullptr;
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint32_t func = RJ_WIN_FUNC(n.out_idx[k]);
            const uint64_t col = RJ_WIN_COL(n.out_idx[k]);
            if (func > RJ_WIN_ROWS_MAX || (func > RJ_WIN_MAX && func < RJ_WIN_LAG)) throw_fmt(RJ_ERR_ARG, "window: unknown function code %u", func);
            int32_t expect = RJ_INT64;
            Out     o{func, (int)col, 0, 0};
            if (func >= RJ_WIN_LAG) {
                if (!args) args = RJ_WINDOW_ARGS(&n);
                if (!args) throw_fmt(RJ_ERR_ARG, "window: function code %u takes an argument but RJ_WINDOW_ARGS is NULL", func);
                o.lo = args[k].lo, o.hi = args[k].hi;
                any_frame = true;
            }
            if (func == RJ_WIN_LAG || func == RJ_WIN_LEAD) {
                if (o.lo < 0 || o.hi != 0)
                    throw_fmt(RJ_ERR_ARG, "window: LAG / LEAD take an offset k >= 0 in arg.lo and 0 in arg.hi (output %llu)", (unsigned long long)k);
                o.lo = o.hi = func == RJ_WIN_LAG ? -o.lo : o.lo;
            } else if (func == RJ_WIN_NTILE) {
                if (o.lo < 1 || o.hi != 0)
                    throw_fmt(RJ_ERR_ARG, "window: NTILE takes a bucket count n >= 1 in arg.lo and 0 in arg.hi (output %llu)", (unsigned long long)k);
            } else if (func >= RJ_WIN_LAG) {
                if (o.lo > o.hi || o.lo == RJ_WIN_UNBOUNDED_FOLLOWING || o.hi == RJ_WIN_UNBOUNDED_PRECEDING)
                    throw_fmt(RJ_ERR_ARG, "window: bad frame (output %llu): lo > hi, lo = UNBOUNDED FOLLOWING or hi = UNBOUNDED PRECEDING",
                              (unsigned long long)k);
            }
            if (func >= RJ_WIN_ROW_NUMBER && func <= RJ_WIN_COUNT_STAR) {
                if (col != 0)
                    throw_fmt(RJ_ERR_ARG, "window: %s takes no column", func == RJ_WIN_COUNT_STAR ? "COUNT(*)" : "a ranking function");
                want[func] = true;
            } else if (func == RJ_WIN_NTILE || func == RJ_WIN_ROWS_COUNT_STAR) {
                if (col != 0) throw_fmt(RJ_ERR_ARG, "window: %s takes no column", func == RJ_WIN_NTILE ? "NTILE" : "COUNT(*)");
            } else {
                if (col >= cw) throw_fmt(RJ_ERR_ARG, "window: output attr out of range");
                const DCol& c = child.cols[col];
                if (func == RJ_WIN_COL) {
                    expect = c.type;
                } else {
                    if (c.type == RJ_VARCHAR)
                        throw_fmt(RJ_ERR_UNSUPPORTED, "window: function over a VARCHAR column (child column %llu): a VARCHAR value "
                                                      "travels as a row id, its pages are not read here", (unsigned long long)col);
                    if ((func == RJ_WIN_SUM || func == RJ_WIN_ROWS_SUM) && c.type == RJ_FP64)
                        throw_fmt(RJ_ERR_UNSUPPORTED, "window: SUM over an FP64 column (child column %llu): a floating-point sum depends "
                                                      "on the order of the rows", (unsigned long long)col);
                    if (func == RJ_WIN_MIN || func == RJ_WIN_MAX || func == RJ_WIN_ROWS_MIN || func == RJ_WIN_ROWS_MAX ||
                        (func >= RJ_WIN_LAG && func <= RJ_WIN_LAST_VALUE))
                        expect = c.type;
                    if (func < RJ_WIN_LAG || func >= RJ_WIN_ROWS_COUNT) {  // (the running count, and what else the function reads)
                        WinCol& w = agg[(int)col];
                        any_peer = any_peer || func < RJ_WIN_LAG;
                        w.want_sum = w.want_sum || func == RJ_WIN_SUM || func == RJ_WIN_ROWS_SUM;
                        w.want_mn = w.want_mn || func == RJ_WIN_MIN;
                        w.want_mx = w.want_mx || func == RJ_WIN_MAX;
                        w.want_tree_mn = w.want_tree_mn || func == RJ_WIN_ROWS_MIN;
                        w.want_tree_mx = w.want_tree_mx || func == RJ_WIN_ROWS_MAX;
                    }
                }
            }
            if (n.out_type[k] != expect) throw_fmt(RJ_ERR_ARG, "window: declared type differs from the function's result type");
            outs.push_back(o);
        }
        check_rows(child);
        if (child.n == 0) return empty_rel(n, root_res);
        const uint32_t rows = (uint32_t)child.n;

        // ---- the order
        const BufP      perm = order_by(child, keys);
        const uint32_t* dperm = ptr<uint32_t>(perm);
        const bool      any_func = std::any_of(outs.begin(), outs.end(), [](const Out& o) { return o.func != RJ_WIN_COL; });
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] window rows=%u keys=%llu partition keys=%llu permuted=%d value columns=%zu\n", rows,
                    (unsigned long long)n_keys, (unsigned long long)n_part, perm ? 1 : 0, agg.size());

        // ---- the heads: P of the partitions, Q of the peer groups; the ranks and the peer ends
        const uint32_t max_chunk = ctx->tune.win_grid > 0 ? (uint32_t)ctx->tune.win_grid : 0u;
        const uint32_t n_quarters = rows / WIN_QUARTER + (rows % WIN_QUARTER != 0);
        BufP           P, Q, rank_col[RJ_WIN_COUNT_STAR + 1], peer_end;
        BufP           part_rowno, part_end;  // every position's partition [i + 1 - part_rowno[i], part_end[i]]
        using ull = unsigned long long;
        if (any_func) {
            const uint64_t mask_bytes = ((uint64_t)rows + 63) / 64 * 8;
            P = ctx->buf(mask_bytes);
            if (part_cols.empty()) launch_win_one_head(L, ptr<ull>(P), rows);
            for (size_t k = 0; k < part_cols.size(); ++k) {
                const DCol& c = child.cols[(size_t)part_cols[k]];
                launch_group_heads(L, c.ref(), dperm, rows, c.type == RJ_FP64, k == 0, false, ptr<ull>(P), nullptr);
            }
            Q = P;  // without order keys every row of a partition is a peer of every other
            if (!order_cols.empty()) {
                Q = ctx->buf(mask_bytes);
                RJ_HIP(hipMemcpyAsync(Q->p, P->p, mask_bytes, hipMemcpyDeviceToDevice, ctx->stream));
                for (int col : order_cols) {
                    const DCol& c = child.cols[(size_t)col];
                    launch_group_heads(L, c.ref(), dperm, rows, c.type == RJ_FP64, false, false, ptr<ull>(Q), nullptr);
                }
            }
            for (uint32_t f = RJ_WIN_ROW_NUMBER; f <= RJ_WIN_COUNT_STAR; ++f)
                if (want[f]) rank_col[f] = ctx->buf((uint64_t)rows * 8);
            // the partitions of the frame layer: k_win_ranks with Q := P, where ROW_NUMBER gives the
            // partition's start and the peer end its end.  Without order keys Q is P: this launch serves.
            const bool ranks_serve = any_frame && order_cols.empty();
            if (ranks_serve && !rank_col[RJ_WIN_ROW_NUMBER]) rank_col[RJ_WIN_ROW_NUMBER] = ctx->buf((uint64_t)rows * 8);
            if (any_peer || ranks_serve) peer_end = ctx->buf((uint64_t)rows * 4);
            BufP           marks[4];
            for (BufP& b : marks) b = ctx->buf((uint64_t)n_quarters * 4);
            const WinMarks m{ptr<uint32_t>(marks[0]), ptr<uint32_t>(marks[1]), ptr<uint32_t>(marks[2]), ptr<uint32_t>(marks[3])};
            const WinRanks r{ptr<ull>(rank_col[RJ_WIN_ROW_NUMBER]), ptr<ull>(rank_col[RJ_WIN_RANK]), ptr<ull>(rank_col[RJ_WIN_DENSE_RANK]),
                             ptr<ull>(rank_col[RJ_WIN_COUNT_STAR]), ptr<uint32_t>(peer_end)};
            launch_win_ranks(L, ptr<ull>(P), ptr<ull>(Q), rows, m, r, max_chunk);
            if (ranks_serve) {
                part_rowno = rank_col[RJ_WIN_ROW_NUMBER], part_end = peer_end;
            } else if (any_frame) {
                part_rowno = ctx->buf((uint64_t)rows * 8), part_end = ctx->buf((uint64_t)rows * 4);
                BufP marks2[4];
                for (BufP& b : marks2) b = ctx->buf((uint64_t)n_quarters * 4);
                const WinMarks m2{ptr<uint32_t>(marks2[0]), ptr<uint32_t>(marks2[1]), ptr<uint32_t>(marks2[2]), ptr<uint32_t>(marks2[3])};
                launch_win_ranks(L, ptr<ull>(P), ptr<ull>(P), rows, m2, WinRanks{ptr<ull>(part_rowno), nullptr, nullptr, nullptr, ptr<uint32_t>(part_end)},
                                 max_chunk);
            }
        }
        const FrameRows frame_rows{ptr<ull>(part_rowno), ptr<uint32_t>(part_end)};

        // ---- the scans: one set of launches per distinct value column
        for (auto& kv : agg) {
            const DCol& c = child.cols[(size_t)kv.first];
            WinCol&     w = kv.second;
            w.nn = ctx->buf((uint64_t)rows * 4);  // (COUNT itself, and what says whether SUM / MIN / MAX are NULL)
            if (w.want_sum) w.sum = ctx->buf((uint64_t)rows * 8);
            if (w.want_mn) w.mn = ctx->buf((uint64_t)rows * 8);
            if (w.want_mx) w.mx = ctx->buf((uint64_t)rows * 8);
            BufP t_head = ctx->buf((uint64_t)n_quarters * 4), t_nn = ctx->buf((uint64_t)n_quarters * 4), t_sum = ctx->buf((uint64_t)n_quarters * 8),
                 t_mn = ctx->buf((uint64_t)n_quarters * 8), t_mx = ctx->buf((uint64_t)n_quarters * 8);
            const WinTails tails{ptr<uint32_t>(t_head), ptr<uint32_t>(t_nn), ptr<ull>(t_sum), ptr<ull>(t_mn), ptr<ull>(t_mx)};
            const WinScan  scan{ptr<uint32_t>(w.nn), ptr<ull>(w.sum), ptr<ull>(w.mn), ptr<ull>(w.mx)};
            launch_win_scan(L, c.ref(), dperm, rows, c.type == RJ_FP64, ptr<ull>(P), tails, scan, max_chunk);
            // ROWS_MIN / ROWS_MAX: one range-extreme tree per (value column, MIN or MAX), shared by all its frames
            if (w.want_tree_mn) {
                w.tree_mn = ctx->buf(frame_tree_words(rows) * 8);
                launch_frame_tree(L, c.ref(), dperm, rows, c.type == RJ_FP64, false, ptr<ull>(w.tree_mn));
            }
            if (w.want_tree_mx) {
                w.tree_mx = ctx->buf(frame_tree_words(rows) * 8);
                launch_frame_tree(L, c.ref(), dperm, rows, c.type == RJ_FP64, true, ptr<ull>(w.tree_mx));
            }
        }

        // ---- the output columns: a passed-through column is gathered once; a function column named several times is
        // made once (func_cols) and, at the root, encoded per output
        // (func_cols; a function from RJ_WIN_LAG on is the same column only under the same argument)
        Sink sink(this, root_res, rows);
        std::map<std::tuple<uint64_t, int64_t, int64_t>, DCol> func_cols;
        for (size_t k = 0; k < outs.size(); ++k) {
            const Out& o = outs[k];
            if (o.func == RJ_WIN_COL) {  // (then the id is the plain column index)
                emit_rows(child, &n.out_idx[k], 1, perm, dperm, sink);
                continue;
            }
            const auto id = std::make_tuple(n.out_idx[k], o.lo, o.hi);
            if (!func_cols.count(id)) {
                if (o.func <= RJ_WIN_COUNT_STAR) {
                    func_cols[id] = dense_col(n.out_type[k], rank_col[o.func]);
                } else if (o.func >= RJ_WIN_LAG) {
                    func_cols[id] = frame_column(child, o.func, o.col, o.lo, o.hi, n.out_type[k], rows, dperm, frame_rows,
                                                 agg.count(o.col) ? &agg.at(o.col) : nullptr);
                } else {
                    const WinCol& w = agg.at(o.col);
                    const DCol&   c = child.cols[(size_t)o.col];
                    const BufP&   src = o.func == RJ_WIN_SUM ? w.sum : (o.func == RJ_WIN_MIN ? w.mn : (o.func == RJ_WIN_MAX ? w.mx : BufP()));
                    // NULL where the frame has no non-NULL value: only a nullable column's frames can
                    const bool nullable = c.valid != nullptr && o.func != RJ_WIN_COUNT;
                    const int  decode = o.func == RJ_WIN_SUM || o.func == RJ_WIN_COUNT
                                            ? GROUP_RAW
                                            : (c.type == RJ_FP64 ? GROUP_KEYF64 : (c.type == RJ_INT32 ? GROUP_KEY32 : GROUP_KEY64));
                    const DCol d = new_col(n.out_type[k], rows, nullable);
                    launch_win_column(L, ptr<ull>(src), ptr<uint32_t>(w.nn), ptr<uint32_t>(peer_end), rows, decode, d.width,
                                      d.hold->as<uint8_t>(), ptr<uint8_t>(d.hold_valid));
                    func_cols[id] = d;
                }
            }
            sink.add(func_cols.at(id));
        }
        return sink.out;
    }

    // ---------------------------------------------------------------------- map
    // RJ_NODE_MAP (semantics in rj.h): computed columns over the one child.  The program is checked and typed
    // by map_check (shared with rj_debug_map_eval), translated into MapProg with one ColRef per RJ_X_COL and
    // the result arrays in its RJ_X_OUT ops, and k_map (rj_map.hip) evaluates ALL expressions in one launch.
    // Passed-through columns are the child's own DCols.  No host sync: the result has the child's rows.
    std::vector<std::unique_ptr<MapProg>> map_progs_;  // the host ends of queued copies: they live as long as the Exec
    ~Exec() {
        if (!map_progs_.empty()) (void)hipStreamSynchronize(ctx->stream);
    }
    Rel map(Rel& child, const rj_node& n, Result* root_res) {
        const size_t      cw = child.cols.size();
        const uint64_t    n_ops = RJ_MAP_N_OPS(&n);
        const rj_expr_op* ops = RJ_MAP_OPS(&n);
        std::vector<int32_t> types(cw);
        std::vector<uint8_t> nullable(cw);
        for (size_t c = 0; c < cw; ++c) {
            types[c] = child.cols[c].type;
            nullable[c] = child.cols[c].valid != nullptr;
        }
        std::vector<MapOp>   dev;
        std::vector<MapExpr> exprs;
        map_check(ops, n_ops, cw, types.data(), nullable.data(), dev, exprs);
        struct ExprOut {
            bool want8 = false, want4 = false;
            DCol d8, d4;
        };
        std::vector<ExprOut> eo(exprs.size());
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint32_t func = RJ_MAP_FUNC(n.out_idx[k]);
            const uint64_t arg = RJ_MAP_ARG(n.out_idx[k]);
            if (func == RJ_MAP_COL) {
                if (arg >= cw) throw_fmt(RJ_ERR_ARG, "map: output attr out of range");
                if (child.cols[arg].type != n.out_type[k])
                    throw_fmt(RJ_ERR_ARG, "map: declared type differs from the child column's type");
            } else if (func == RJ_MAP_EXPR) {
                if (arg >= exprs.size())
                    throw_fmt(RJ_ERR_ARG, "map: output %llu names expression %llu, the program holds %zu", (unsigned long long)k,
                              (unsigned long long)arg, exprs.size());
                const int32_t t = n.out_type[k];
                if (exprs[arg].f64 ? t != RJ_FP64 : (t != RJ_INT64 && t != RJ_INT32))
                    throw_fmt(RJ_ERR_ARG, "map: declared type differs from the expression's type (an I64 expression is INT64 or INT32, "
                                          "an F64 one FP64)");
                (t == RJ_INT32 ? eo[arg].want4 : eo[arg].want8) = true;
            } else {
                throw_fmt(RJ_ERR_ARG, "map: unknown output code %u", func);
            }
        }
        for (size_t e = 0; e < eo.size(); ++e)
            if (!eo[e].want8 && !eo[e].want4) throw_fmt(RJ_ERR_ARG, "map: no output names expression %zu", e);
        check_rows(child);
        if (child.n == 0) return empty_rel(n, root_res);
        const uint64_t rows = child.n;

        // ---- the device program: the columns it reads, the arrays it writes
        if (!exprs.empty()) {
            map_progs_.emplace_back(new MapProg());
            MapProg& prog = *map_progs_.back();
            size_t   e = 0;
            for (uint64_t k = 0; k < n_ops; ++k) {
                MapOp& o = dev[k];
                if (o.op == X_COL) o.a = child.cols[(size_t)ops[k].column].ref();
                if (o.op == X_OUT) {
                    ExprOut& x = eo[e];
                    BufP     valid = exprs[e].nullable ? ctx->buf(rows) : BufP();  // (one array under both types)
                    if (x.want8) x.d8 = dense_col(exprs[e].f64 ? RJ_FP64 : RJ_INT64, ctx->buf(rows * 8), valid);
                    if (x.want4) x.d4 = dense_col(RJ_INT32, ctx->buf(rows * 4), valid);
                    o.out8 = ptr<uint8_t>(x.d8.hold);
                    o.out4 = ptr<uint8_t>(x.d4.hold);
                    o.valid = ptr<uint8_t>(valid);
                    ++e;
                }
                prog.ops[k] = o;
            }
            BufP           dprog = ctx->buf(sizeof(MapProg));
            const uint64_t tiles = (rows + MAP_TILE - 1) / MAP_TILE;
            uint64_t       grid = std::min<uint64_t>(tiles, (uint64_t)ctx->compute_units() * 8);
            if (ctx->tune.map_grid > 0) grid = std::min<uint64_t>(grid, (uint64_t)ctx->tune.map_grid);
            RJ_HIP(hipMemcpyAsync(dprog->p, &prog, n_ops * sizeof(MapOp), hipMemcpyHostToDevice, ctx->stream));
            launch_map(L, dprog->as<MapProg>(), (uint32_t)n_ops, (uint32_t)rows, (uint32_t)grid);
        }
        if (ctx->tune.diag >= 2)
            fprintf(stderr, "[rj diag] map rows=%llu ops=%llu expressions=%zu\n", (unsigned long long)rows, (unsigned long long)n_ops,
                    exprs.size());

        // ---- the output columns: a passed-through column is the child's own (at the root through the writers of a
        // projection); an expression named twice under one type is encoded once: the id says which of its two arrays.
        // The ids of the arrays lie above every column index (RJ_MAP_ARG keeps 56 bits), whatever RJ_MAP_* codes exist.
        const uint64_t expr_ids = 1ull << 56;
        Sink           sink(this, root_res, rows);
        for (uint64_t k = 0; k < n.n_out; ++k) {
            const uint64_t arg = RJ_MAP_ARG(n.out_idx[k]);
            const bool     narrow = n.out_type[k] == RJ_INT32;
            if (RJ_MAP_FUNC(n.out_idx[k]) == RJ_MAP_COL)
                emit_rows(child, &arg, 1, BufP(), nullptr, sink);
            else
                sink.add(expr_ids + arg * 2 + narrow, [&] { return narrow ? eo[arg].d4 : eo[arg].d8; });
        }
        return sink.out;
    }

    // ------------------------------------------------------------- a node's output
    // A column of `rows` rows as a root result column: Page images.  The strings of a VARCHAR column are
    // gathered through its row ids, a column that emit_rows gathered into Page images is handed over, and
    // any other fixed-width column (paged, or dense with or without validity) is encoded on the device.
    ResultColumn col_to_result(const DCol& d, uint64_t rows) {
        ResultColumn rc;
        rc.type = d.type;
        if (d.type == RJ_VARCHAR) {
            BufP            rowids;
            const uint32_t* ids = reinterpret_cast<const uint32_t*>(d.ptr);
            if (d.kind == COL_IOTA) {  // (a projection only: every row of the base table, in order)
                rowids = ctx->buf(rows * 4);
                launch_gather(L, d.ref(), nullptr, rows, OutStream{rowids->as<uint8_t>(), ST_DENSE32, 0}, nullptr);
                ids = rowids->as<uint32_t>();
            }
            varchar_root(ids, rows, d, rc);
        } else if (d.kind == COL_PAGED && d.hold) {  // (a table's own pages have no holder)
            rc.dev_pages = d.hold;
            rc.n_pages = pages_for(rows, d.width);
        } else if (rows) {
            rc.n_pages = pages_for(rows, d.width);
            rc.dev_pages = ctx->buf(rc.n_pages * PAGE_BYTES);
            if (d.valid) {
                launch_encode_nullable(L, d.ptr, d.valid, rows, d.width, rc.dev_pages->as<uint8_t>());
            } else {
                launch_gather(L, d.ref(), nullptr, rows,
                              OutStream{rc.dev_pages->as<uint8_t>(), d.width == 4 ? ST_PAGED32 : ST_PAGED64, 0}, nullptr);
                launch_finish_pages(L, rc.dev_pages->as<uint8_t>(), rows, d.width);
            }
        }
        return rc;
    }
    static int stream_mode_of(bool is_root, int width, bool direct_output) {
        if (is_root && direct_output) return width == 4 ? ST_PAGED32 : ST_PAGED64;
        return width == 4 ? ST_DENSE32 : ST_DENSE64;
    }
    static uint64_t stream_bytes(int mode, uint64_t rows) {
        switch (mode) {
        case ST_DENSE32: return rows * 4;
        case ST_DENSE64: return rows * 8;
        case ST_PAGED32: return pages_for(rows, 4) * PAGE_BYTES;
        case ST_PAGED64: return pages_for(rows, 8) * PAGE_BYTES;
        case ST_DENSE96: return rows * 12;
        default: return 0;
        }
    }
    // the layout of each side's carry stream
    static void plan_carry_streams(JoinState& st) {
        for (Side* s : {&st.ls, &st.rs}) {
            if (s->carry_mode == CARRY_NONE)
                s->stream_mode = ST_NONE;
            else if (s->carry_mode == CARRY_ROWIDX)
                s->stream_mode = ST_DENSE32;
            else if (s->carry_mode == CARRY_WIDE)
                s->stream_mode = s->CW == 2 ? ST_DENSE64 : ST_DENSE96;  // records, split below
            else {
                const DCol& c = s->rel->cols[s->carry_col];
                s->stream_mode = stream_mode_of(st.is_root, c.width, c.type != RJ_VARCHAR);
            }
        }
    }
    // headers + bitmaps of the streams a probe wrote straight into Page images, from the row count
    // on the device (counters[0]); e.finished records them
    void finish_paged_streams(JoinState& st, Emitted& e, const BufP& counters, uint64_t cap) {
        uint8_t* fp[3];
        int      fw[3];
        uint32_t nf = 0;
        auto add = [&](const BufP& b, int mode) {
            if (!b || (mode != ST_PAGED32 && mode != ST_PAGED64) || e.finished.count(b->p)) return;
            fp[nf] = b->as<uint8_t>();
            fw[nf] = mode == ST_PAGED32 ? 4 : 8;
            ++nf;
            e.finished.insert(b->p);
        };
        add(e.key_stream, e.key_mode);
        add(st.ls.stream, st.ls.stream_mode);
        add(st.rs.stream, st.rs.stream_mode);
        launch_finish_streams(L, fp, fw, nf, counters->as<unsigned long long>(), cap);
    }

    // What the probe's streams become: wide records split into columns, row-index carries gathered,
    // and at the root Page images (late materialisation; shared by every kind of join).
    Rel join_assemble(JoinState& st, const JoinSpec& js, Emitted& e, Result* root_res) {
        Side &         ls = st.ls, &rs = st.rs;
        const size_t   lw = st.lw;
        const bool     is_root = st.is_root;
        const uint64_t nrows = e.nrows;

        // wide carries: the emitted records -> one dense array (+ validity bytes) per column
        for (Side* s : {&ls, &rs}) {
            if (s->carry_mode != CARRY_WIDE) continue;
            SplitParams sp{};
            sp.rec = s->stream->as<uint32_t>();
            sp.cw = (uint32_t)s->CW;
            sp.valid_word = s->valid_word;
            int word = 0;
            for (size_t i = 0; i < s->wide_cols.size(); ++i) {
                const DCol&   col = s->rel->cols[s->wide_cols[i]];
                Side::WideOut wo;
                // a root column without NULLs goes into its Page images here (the header words are
                // filled in below), anything else into a dense array
                const bool nullable = s->nullable(s->wide_cols[i]);  // (here, or on another rank of a sharded join)
                const bool to_pages = is_root && !nullable && col.type != RJ_VARCHAR;  // (a VARCHAR column travels as row ids)
                wo.mode = to_pages ? (col.width == 4 ? ST_PAGED32 : ST_PAGED64) : (col.width == 4 ? ST_DENSE32 : ST_DENSE64);
                wo.values = ctx->buf(stream_bytes(wo.mode, std::max<uint64_t>(nrows, 1)));
                if (nullable) wo.valid = ctx->buf(std::max<uint64_t>(nrows, 1));
                sp.col[i].out = wo.values->as<uint8_t>();
                sp.col[i].valid = ptr<uint8_t>(wo.valid);
                sp.col[i].word = word;
                sp.col[i].width = col.width;
                sp.col[i].valid_bit = (int32_t)i;
                sp.col[i].paged = to_pages ? 1 : 0;
                word += col.width / 4;
                s->wide_out[s->wide_cols[i]] = wo;
            }
            sp.n_cols = (int32_t)s->wide_cols.size();
            launch_split_records(L, sp, nrows);
        }

        // ------------------------------------------------ assemble the outputs
        Rel out;
        out.n = nrows;
        if (is_root) root_res->num_rows = nrows;
        for (size_t k = 0; k < js.out_idx.size(); ++k) {
            bool        is_left = js.out_idx[k] < lw;
            Side&       s = is_left ? ls : rs;
            int         c = (int)(is_left ? js.out_idx[k] : js.out_idx[k] - lw);
            const DCol& src = s.rel->cols[c];
            BufP buf;           // where this column's values/pages live
            int  buf_mode = ST_NONE;
            BufP valid;
            if ((uint64_t)c == s.key_col && st.need_key_stream && !s.optional) {
                buf = e.key_stream;
                buf_mode = e.key_mode;
            } else if (s.carry_mode == CARRY_COLUMN) {
                buf = s.stream;
                buf_mode = s.stream_mode;
            } else if (s.carry_mode == CARRY_WIDE) {
                const Side::WideOut& wo = s.wide_out.at(c);
                buf = wo.values;
                valid = wo.valid;
                buf_mode = wo.mode;
            } else {
                // generic path: gather the child column through the row-index stream
                const uint32_t* idx = s.stream->as<uint32_t>();
                if (s.optional) {
                    // an outer join's optional side: the row ids of padded rows are OUTER_NO_ROW, which
                    // k_outer_gather turns into NULLs without reading a row (the relation may be empty)
                    buf_mode = src.width == 4 ? ST_DENSE32 : ST_DENSE64;
                    buf = ctx->buf(stream_bytes(buf_mode, std::max<uint64_t>(nrows, 1)));
                    valid = ctx->buf(std::max<uint64_t>(nrows, 1));
                    launch_outer_gather(L, src.ref(), idx, nrows, buf->as<uint8_t>(), valid->as<uint8_t>());
                } else if (src.kind == COL_IOTA) {
                    buf = s.stream;  // row ids of the base table ARE the stream
                    buf_mode = ST_DENSE32;
                } else {
                    bool to_pages = is_root && src.type != RJ_VARCHAR && src.valid == nullptr;
                    buf_mode = to_pages ? (src.width == 4 ? ST_PAGED32 : ST_PAGED64)
                                        : (src.width == 4 ? ST_DENSE32 : ST_DENSE64);
                    buf = ctx->buf(stream_bytes(buf_mode, std::max<uint64_t>(nrows, 1)));
                    if (src.valid) valid = ctx->buf(std::max<uint64_t>(nrows, 1));
                    launch_gather(L, src.ref(), idx, nrows,
                                  OutStream{buf->as<uint8_t>(), buf_mode, 0}, ptr<uint8_t>(valid));
                }
            }
            if (!is_root) {
                out.cols.push_back(dense_like(src, buf, valid));
                continue;
            }
            // ---- root: Page images (replaces Table::to_columnar, build_table.cpp:456-681)
            ResultColumn rc;
            rc.type = src.type;
            if (nrows == 0) {
                // empty result: typed columns with zero pages (reference tests/unit_tests.cpp:24-27)
            } else if (src.type == RJ_VARCHAR) {
                varchar_root(buf->as<uint32_t>(), nrows, src, rc);
            } else if (buf_mode == ST_PAGED32 || buf_mode == ST_PAGED64) {
                if (!e.finished.count(buf->p)) {
                    launch_finish_pages(L, buf->as<uint8_t>(), nrows, src.width);
                    e.finished.insert(buf->p);
                }
                rc.dev_pages = buf;
                rc.n_pages = pages_for(nrows, src.width);
            } else {
                // dense values (+ validity): encode pages on the device
                rc.n_pages = pages_for(nrows, src.width);
                rc.dev_pages = ctx->buf(rc.n_pages * PAGE_BYTES);
                if (valid) {
                    launch_encode_nullable(L, buf->as<uint8_t>(), valid->as<uint8_t>(), nrows,
                                           src.width, rc.dev_pages->as<uint8_t>());
                } else {
                    launch_gather(L, dense_like(src, buf).ref(), nullptr, nrows,
                                  OutStream{rc.dev_pages->as<uint8_t>(),
                                            src.width == 4 ? ST_PAGED32 : ST_PAGED64, 0},
                                  nullptr);
                    launch_finish_pages(L, rc.dev_pages->as<uint8_t>(), nrows, src.width);
                }
            }
            root_res->cols.push_back(std::move(rc));
        }
        return out;
    }

    // The page directory (rows before each page) of VARCHAR column vc_col of table vc_table, built on
    // first use; a column whose pages the reference refuses leaves no entry behind.
    const std::vector<uint64_t>& vc_directory(int vc_table, int vc_col, const Table* t) {
        auto key = std::make_pair(vc_table, vc_col);
        auto it = vc_dir_.find(key);
        if (it == vc_dir_.end()) {
            const TableColumn&    tc = t->cols[vc_col];
            std::vector<uint64_t> dir;
            varchar_dir_build(tc.vc_pages.data(), tc.vc_pages.size(), t->num_rows, dir);
            it = vc_dir_.emplace(key, std::move(dir)).first;
        }
        return it->second;
    }

    // The VARCHAR pages of a base column + their row directory in HBM (uploaded once per table).
    struct VcDev {
        const uint8_t*  pages;
        uint32_t        n_pages;
        const uint32_t* dir;
    };
    VcDev ensure_vc_dev(int vc_table, int vc_col) {
        if (vc_table < 0 || (uint64_t)vc_table >= n_tables) throw_fmt(RJ_ERR_ARG, "VARCHAR column without provenance");
        const Table*       t = table_by_id((uint64_t)vc_table);
        const TableColumn& tc = t->cols[vc_col];
        if (tc.vc_pages.size() > 0xfffffff0ull || t->num_rows > 0xfffffff0ull)
            throw_fmt(RJ_ERR_UNSUPPORTED, "VARCHAR column too large for the device path");
        const std::vector<uint64_t>& dir = vc_directory(vc_table, vc_col, t);
        const uint32_t npg = (uint32_t)tc.vc_pages.size();
        if (!tc.vc_dev) {  // (a table ingested on the device brings its pages along: rj_ingest.hip)
            tc.vc_dev = ctx->buf(std::max<uint64_t>(npg, 1) * PAGE_BYTES);
            upload_host_pages(ctx, tc.vc_pages.data(), npg, tc.vc_dev->as<uint8_t>());
        }
        if (!tc.vc_dev_dir) {
            std::vector<uint32_t> dir32(dir.begin(), dir.end());
            tc.vc_dev_dir = ctx->buf(dir32.size() * 4);
            RJ_HIP(hipMemcpyAsync(tc.vc_dev_dir->p, dir32.data(), dir32.size() * 4, hipMemcpyHostToDevice,
                                  ctx->stream));
            ctx->sync();  // dir32 is a local
        }
        return VcDev{tc.vc_dev->as<uint8_t>(), npg, tc.vc_dev_dir->as<uint32_t>()};
    }

    // VARCHAR join keys: hash both key columns, join on the hashes (see JoinState::VKey)
    void hash_varchar_keys(JoinState& st) {
        int k = 0;
        for (Side* s : {&st.ls, &st.rs}) {
            JoinState::VKey& v = st.vk[k++];
            const DCol       kc = s->rel->cols[s->key_col];  // a row-id column of its base table
            if (kc.kind != COL_IOTA && kc.kind != COL_DENSE) throw_fmt(RJ_ERR_ARG, "VARCHAR key column of unknown shape");
            const VcDev d = ensure_vc_dev(kc.vc_table, kc.vc_col);
            const uint32_t n = (uint32_t)s->rel->n;
            v.pages = d.pages;
            v.n_pages = d.n_pages;
            v.rows = ctx->buf(std::max<uint64_t>(n, 1) * sizeof(VcRow));
            v.hash = ctx->buf(std::max<uint64_t>(n, 1) * 8);
            v.valid = ctx->buf(std::max<uint64_t>(n, 1));
            launch_vc_hash(L, d.pages, d.n_pages, d.dir,
                           kc.kind == COL_DENSE ? reinterpret_cast<const uint32_t*>(kc.ptr) : nullptr, n,
                           v.rows->as<VcRow>(), v.hash->as<uint64_t>(), v.valid->as<uint8_t>(),
                           ctx->tune.vkey_hash_bits > 0 && ctx->tune.vkey_hash_bits < 64
                               ? ((1ull << ctx->tune.vkey_hash_bits) - 1ull)
                               : ~0ull);
            v.rel = *s->rel;
            v.rel.cols.push_back(dense_col(RJ_INT64, v.hash, v.valid));
            s->rel = &v.rel;
            s->key_col = v.rel.cols.size() - 1;
        }
    }

    // Every joined pair is compared byte for byte; the (build row, probe row) streams are
    // compacted if — and only if — a hash collision let a pair of different strings through.
    uint64_t verify_varchar_pairs(JoinState& st, uint64_t nrows) {
        Side &                 bs = st.bs(), &ps = st.ps();
        const JoinState::VKey& vb = st.vk[st.build_left ? 0 : 1];
        const JoinState::VKey& vp = st.vk[st.build_left ? 1 : 0];
        const uint32_t         n = (uint32_t)nrows;
        BufP                   keep = ctx->buf(n), bad = ctx->buf(16);
        RJ_HIP(hipMemsetAsync(bad->p, 0, 16, ctx->stream));
        launch_vc_verify(L, vb.pages, vb.n_pages, vb.rows->as<VcRow>(), vp.pages, vp.n_pages, vp.rows->as<VcRow>(),
                         bs.stream->as<uint32_t>(), ps.stream->as<uint32_t>(), n, keep->as<uint8_t>(),
                         bad->as<unsigned long long>());
        unsigned long long n_bad = 0;
        read_back(&n_bad, bad->p, 8);
        if (n_bad == 0) return nrows;
        BufP nb = ctx->buf(std::max<uint64_t>(nrows - n_bad, 1) * 4), np = ctx->buf(std::max<uint64_t>(nrows - n_bad, 1) * 4);
        launch_vc_compact(L, keep->as<uint8_t>(), bs.stream->as<uint32_t>(), ps.stream->as<uint32_t>(), n,
                          nb->as<uint32_t>(), np->as<uint32_t>(), bad->as<unsigned long long>() + 1);
        bs.stream = nb;
        ps.stream = np;
        return nrows - n_bad;
    }

    void launch_heavy_tasks_zeroed(const Parted& PB, const Parted& PP, const BufP& tasks,
                                   const BufP& counters, uint32_t max_tasks) {
        RJ_HIP(hipMemsetAsync(counters->p, 0, 16, ctx->stream));
        launch_heavy_tasks(L, PB.off->as<uint32_t>(), PP.off->as<uint32_t>(), PB.NP,
                           tasks->as<uint32_t>(), counters->as<uint32_t>() + 2, max_tasks, PB.off_shift | (PP.off_shift << 1));
    }

    // VARCHAR at the root: row ids -> host, strings gathered from the base table's
    // pages and encoded with the reference's fill rule (build_table.cpp:595-677).
    void varchar_root(const uint32_t* dev_rowids, uint64_t n, const DCol& src, ResultColumn& rc) {
        if (src.vc_table < 0 || (uint64_t)src.vc_table >= n_tables)
            throw_fmt(RJ_ERR_ARG, "VARCHAR column without provenance");
        const Table*       t = table_by_id((uint64_t)src.vc_table);
        const TableColumn& tc = t->cols[src.vc_col];
        const bool diag = ctx->tune.diag >= 2;
        auto       tv0 = std::chrono::steady_clock::now();
        if (ctx->tune.varchar_dev_rows > 0 && n >= (uint64_t)ctx->tune.varchar_dev_rows &&
            tc.vc_pages.size() <= 0xfffffff0ull && t->num_rows <= 0xfffffff0ull) {
            // ---- large result: gather + encode on the device (rj_varchar_dev.hip)
            const VcDev    vd = ensure_vc_dev(src.vc_table, src.vc_col);
            const uint32_t npg = vd.n_pages;
            auto           tv1 = std::chrono::steady_clock::now();
            const uint32_t nr = (uint32_t)n, chunks = (nr + VC_CHUNK - 1) / VC_CHUNK;
            BufP           vrows = ctx->buf((uint64_t)nr * sizeof(VcRow));
            BufP           pcnt = ctx->buf((uint64_t)chunks * 4), pbase = ctx->buf(((uint64_t)chunks + 1) * 4);
            launch_vc_resolve(L, vd.pages, npg, vd.dir, dev_rowids, nr, vrows->as<VcRow>());
            launch_vc_walk(L, vrows->as<VcRow>(), nr, pcnt->as<uint32_t>(), nullptr, nullptr);
            launch_scan_bins(L, pcnt->as<uint32_t>(), chunks, pbase->as<uint32_t>(), nullptr);
            uint32_t n_out = 0;
            read_back(&n_out, pbase->as<uint32_t>() + chunks, 4);
            BufP plist = ctx->buf(std::max<uint64_t>(n_out, 1) * sizeof(VcPage));
            rc.dev_pages = ctx->buf(std::max<uint64_t>(n_out, 1) * PAGE_BYTES);
            launch_vc_walk(L, vrows->as<VcRow>(), nr, pcnt->as<uint32_t>(), pbase->as<uint32_t>(),
                           plist->as<VcPage>());
            launch_vc_encode(L, vd.pages, npg, vrows->as<VcRow>(), plist->as<VcPage>(), n_out,
                             rc.dev_pages->as<uint8_t>());
            rc.n_pages = n_out;
            if (diag) {
                ctx->sync();
                auto tv2 = std::chrono::steady_clock::now();
                auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                fprintf(stderr, "[rj host]   varchar col on the device: %llu rows -> %u pages, source pages in HBM %.2f ms, resolve+walk+encode %.2f ms\n",
                        (unsigned long long)n, n_out, ms(tv0, tv1), ms(tv1, tv2));
            }
            return;
        }
        std::vector<uint32_t> ids(n);
        read_back(ids.data(), dev_rowids, n * 4);
        auto tv1 = std::chrono::steady_clock::now();
        const std::vector<uint64_t>& dir = vc_directory(src.vc_table, src.vc_col, t);
        auto tv2 = std::chrono::steady_clock::now();
        varchar_gather_encode(tc.vc_pages.data(), tc.vc_pages.size(), dir, ids.data(), n,
                              rc.host_pages, rc.n_pages);
        if (diag) {
            auto tv3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "[rj host]   varchar col: %llu rows, wait+D2H %.2f ms, page directory %.2f ms, gather+encode %.2f ms\n",
                    (unsigned long long)n, ms(tv0, tv1), ms(tv1, tv2), ms(tv2, tv3));
        }
    }
};


// ================================================================ sharded executor
// One JoinNode across the ranks of a job: every rank
//   stage A   forms (hashed key, carry) tuples of its shard of both children and partitions them
//             by (OWNER rank = top log2(world) hash bits, first local digit = low bits) in ONE radix
//             pass (fan-out = world x 2^s <= 512; RJ_TUNE_FOLD_OWNER=0: by owner only);
//   exchange  ONE variable-size all-to-all per relation (rj_comm: peer copies or RCCL), on its own
//             stream — the build side's exchange overlaps the probe side's stage A, the probe side's
//             the build side's stage B; its layout is host arithmetic over the all-gathered counts
//             (rj_xplan.cpp);
//   stage B   runs the remaining radix passes + build/probe on what arrived (the runs of a digit as
//             input segments of its first pass), i.e. the single-device join on an N-th of the data.
// Results stay on the owning rank (no reduction).  One host thread drives all local ranks phase by
// phase; everything between the count read-backs is asynchronous.  What a rank decides from its own
// DATA and that shapes what is exchanged (which columns need a validity word) is agreed on first;
// local failures travel as status words with the counts, and every wait on a peer is bounded.
class ShardedExec {
   public:
    ShardedExec(Context* group, const rj_plan* plan, Table* const* tables, uint64_t n_inputs, int flags)
        : g_(group), plan_(plan), nl_(group->n_lanes()) {
        if (!plan || plan->root >= plan->n_nodes) throw_fmt(RJ_ERR_ARG, "bad plan root");
        comm_ = group->comm.get();
        world_ = comm_ ? comm_->world() : 1;
        rank_base_ = comm_ ? comm_->rank_base() : 0;
        rb_ = ceil_log2((uint64_t)world_);
        for (int l = 0; l < nl_; ++l) {
            Context* c = group->lane(l);
            for (uint64_t i = 0; i < n_inputs; ++i) {
                Table* t = tables[(size_t)l * n_inputs + i];
                if (!t) throw_fmt(RJ_ERR_ARG, "null table");
                if (t->ctx != c) throw_fmt(RJ_ERR_ARG, "table %llu of device %d lives on another device's context",
                                           (unsigned long long)i, l);
            }
            ex_.emplace_back(new Exec(c, plan, tables + (size_t)l * n_inputs, n_inputs, flags));
        }
    }

    void run(Result** out) {
        std::vector<std::unique_ptr<Result>> res;
        for (int l = 0; l < nl_; ++l) {
            res.emplace_back(new rj_result());
            res.back()->ctx = g_->lane(l);
        }
        std::vector<Result*> rp;
        for (auto& r : res) rp.push_back(r.get());
        const rj_node& root = plan_->nodes[plan_->root];
        try {
            if (root.kind == RJ_NODE_SCAN) {
                for (int l = 0; l < nl_; ++l) {
                    use(l);
                    ex_[l]->root_scan(root, *res[l]);
                }
            } else {
                (void)node(plan_->root, &rp, 0);
            }
            for (const LocalErr& e : pending_)  // (a failure of the last join's local part)
                if (e.code) throw rj::Error(e.code, e.msg);
            sync_all();
        } catch (...) {
            // kernels and copies still queued may reference buffers about to be released
            // (compute streams never wait on an unfinished exchange — see stage B — so they drain;
            // the exchange streams are waited for with the transport's bound, unless it gave up)
            for (int l = 0; l < nl_; ++l) {
                (void)hipSetDevice(g_->lane(l)->device);
                (void)hipStreamSynchronize(g_->lane(l)->stream);
                if (comm_ && !comm_->failed()) {
                    try {
                        comm_->wait_stream(l, "the exchange streams (after an error)");
                    } catch (...) {
                    }
                }
            }
            (void)hipSetDevice(g_->device);
            throw;
        }
        use(0);
        for (int l = 0; l < nl_; ++l) out[l] = res[l].release();
    }

   private:
    Context*                           g_;
    const rj_plan*                     plan_;
    int                                nl_, world_ = 1, rank_base_ = 0;
    uint32_t                           rb_ = 0;
    Comm*                              comm_ = nullptr;
    std::vector<std::unique_ptr<Exec>> ex_;

    void use(int l) { RJ_HIP(hipSetDevice(g_->lane(l)->device)); }
    void sync_all() {
        for (int l = 0; l < nl_; ++l) {
            use(l);
            g_->lane(l)->sync();
        }
    }

    using Ev = Event;  // (made on a lane's device)

    std::vector<Rel> node(uint64_t idx, std::vector<Result*>* root_res, int depth) {
        if (idx >= plan_->n_nodes) throw_fmt(RJ_ERR_ARG, "bad node index");
        if (depth > 4096) throw_fmt(RJ_ERR_ARG, "plan too deep (cycle?)");
        const rj_node& n = plan_->nodes[idx];
        if (n.kind == RJ_NODE_SCAN) {
            // a scan that fails on one rank (its shard's pages are malformed: "row_idx") must not
            // leave the other ranks waiting in the next join's collectives: the error is kept and
            // travels as that join's first status word
            std::vector<Rel> r((size_t)nl_);
            if (pending_.empty()) pending_.resize((size_t)nl_);
            for (int l = 0; l < nl_; ++l)
                guarded(pending_[l], [&] {
                    use(l);
                    inject_failure(5, l);
                    r[l] = ex_[l]->scan(n);
                });
            return r;
        }
        // (execute_sharded has refused the kinds that do not run sharded: first_unshardable)
        if (n.kind != RJ_NODE_JOIN) throw_fmt(RJ_ERR_ARG, "bad node kind");
        std::vector<Rel> L = node(n.left, nullptr, depth + 1);
        std::vector<Rel> R = node(n.right, nullptr, depth + 1);
        return join(L, R, join_spec(n, g_->radix_bits_override), root_res);
    }

    // bytes per tuple of array `a` in the partition layout, 0 = no such array
    static uint32_t array_width(const Parted& P, int KW, int CW, int a) {
        if (P.packed) return a == 0 ? 8u : 0u;
        if (a >= P.NW) return 0;
        const int pw = CW >= 2 ? KW + CW - 2 : -1;  // the last two carry words are one pair array
        if (pw >= 0 && a == pw + 1) return 0;
        return a == pw ? 8u : 4u;
    }

    // A local failure on one rank must not leave its peers blocked in a collective: every rank
    // reports a status word with the counts it all-gathers anyway, and ALL ranks give up together,
    // before any data moves.  The failing rank rethrows its own error, the others name it.
    struct LocalErr {
        int         code = 0;
        std::string msg;
    };
    std::vector<LocalErr> pending_;  // per local rank: a scan's failure, waiting for the next join's status word
    template <class F>
    static void guarded(LocalErr& e, F&& f) {
        if (e.code) return;  // this rank failed earlier: it only keeps the collectives company
        try {
            f();
        } catch (const rj::Error& x) {
            e.code = x.code ? x.code : RJ_ERR_DEVICE;
            e.msg = x.what();
        } catch (const std::bad_alloc&) {
            e.code = RJ_ERR_NOMEM;
            e.msg = "host allocation failed";
        } catch (const std::exception& x) {
            e.code = RJ_ERR_DEVICE;
            e.msg = x.what();
        }
    }
    void agree(const std::vector<std::vector<uint64_t>>& all, size_t status_at, const std::vector<LocalErr>& lerr,
               const char* doing) {
        int bad = -1;
        for (int r = 0; r < world_ && bad < 0; ++r)
            if (all[r][status_at] != 0) bad = r;
        if (bad < 0) return;
        for (int l = 0; l < nl_; ++l)
            if (lerr[l].code) throw rj::Error(lerr[l].code, lerr[l].msg);
        throw_fmt(RJ_ERR_DEVICE, "sharded join: rank %d failed (status %llu) while %s; every rank gives up before the exchange",
                  bad, (unsigned long long)all[bad][status_at], doing);
    }
    void inject_failure(int at, int lane) {
        if (g_->tune.debug_shard_fail == at && g_->tune.debug_shard_fail_rank == rank_base_ + lane)
            throw_fmt(RJ_ERR_NOMEM, "injected failure %d on rank %d (RJ_DEBUG_SHARD_FAIL)", at, rank_base_ + lane);
    }
    void wait_xfer(int l, const char* what) {
        if (comm_) comm_->wait_stream(l, what);
    }

    std::vector<Rel> join(std::vector<Rel>& left, std::vector<Rel>& right, const JoinSpec& js,
                          std::vector<Result*>* root_res) {
        std::vector<Exec::JoinState> st((size_t)nl_);
        const bool diag = g_->tune.diag >= 2;
        auto       t_start = std::chrono::steady_clock::now();
        auto       lap = [&](const char* what) {
            if (!diag) return;
            sync_all();
            for (int l = 0; l < nl_; ++l) wait_xfer(l, what);
            auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "[rj sharded] rank %d: %-28s %8.2f ms\n", rank_base_, what,
                    std::chrono::duration<double, std::milli>(now - t_start).count());
            t_start = now;
        };
        // ---- what every rank decides locally, then agrees on globally
        std::vector<LocalErr>              lerr((size_t)nl_);
        if (!pending_.empty()) lerr = pending_;  // (a scan below this join failed on a local rank)
        std::vector<std::vector<uint64_t>> mine((size_t)nl_), all;
        // which columns hold NULLs on ANY rank: the carry layout (a validity word or not, one column
        // as it is or value + validity) follows the data, and every rank must pick the same one
        uint64_t shared_nulls[2] = {0, 0};
        for (int l = 0; l < nl_; ++l) mine[l] = {Exec::null_columns(left[l]), Exec::null_columns(right[l])};
        gather(mine, 2, all);
        for (int r = 0; r < world_; ++r) {
            shared_nulls[0] |= all[r][0];
            shared_nulls[1] |= all[r][1];
        }
        for (int l = 0; l < nl_; ++l) {
            bool ok = true;
            guarded(lerr[l], [&] {
                use(l);
                inject_failure(1, l);
                ex_[l]->join_prepare(left[l], right[l], js, root_res != nullptr, st[l], join_kind(RJ_NODE_JOIN), shared_nulls);
                for (Exec::Side* s : {&st[l].ls, &st[l].rs}) {
                    if (s->carry_mode == CARRY_ROWIDX) ok = false;  // a row index means nothing on another rank
                    if (s->carry_mode == CARRY_COLUMN && s->rel->cols[s->carry_col].kind == COL_IOTA) ok = false;
                    if (s->carry_mode == CARRY_WIDE)
                        for (int c : s->wide_cols)
                            if (s->rel->cols[c].kind == COL_IOTA || s->rel->cols[c].type == RJ_VARCHAR) ok = false;
                    ex_[l]->prepare_wide(*s);
                }
            });
            mine[l] = {left[l].n, right[l].n, ok ? 1ull : 0ull, (uint64_t)lerr[l].code};
        }
        gather(mine, 4, all);
        agree(all, 3, lerr, "preparing the join");
        uint64_t tot_left = 0, tot_right = 0;
        bool     ok = true;
        for (int r = 0; r < world_; ++r) {
            tot_left += all[r][0];
            tot_right += all[r][1];
            ok = ok && all[r][2] != 0;
        }
        auto all_empty = [&] {
            std::vector<Rel> out((size_t)nl_);
            for (int l = 0; l < nl_; ++l) {
                use(l);
                out[l] = ex_[l]->empty_rel(js, root_res ? (*root_res)[l] : nullptr);
            }
            return out;
        };
        // with an empty child the reference returns {} before looking at anything
        // (src/execute.cpp:50); a probe key of another type matches nothing (:65-71)
        if (tot_left == 0 || tot_right == 0 || st[0].type_mismatch) return all_empty();
        if (!ok)
            throw_fmt(RJ_ERR_UNSUPPORTED,
                      "sharded join: a side needs more payload than travels with the key (more than %d carry "
                      "words incl. a validity word, or a VARCHAR column): its row index would travel, and "
                      "means nothing on another rank",
                      MAX_WORDS - st[0].KW);
        const int KW = st[0].KW;

        // ---- the radix plan, from totals every rank knows: L local bits per rank, of which the
        // first digit (s bits) rides on stage A's pass together with the owner digit (rb_ bits) —
        // stage A fans out world * 2^s ways, and stage B starts at the second local digit
        const uint64_t tot_build = js.build_left ? tot_left : tot_right;
        const uint32_t Lbits = ex_[0]->join_bits(js, std::max<uint64_t>((tot_build + world_ - 1) / world_, 1), rb_);
        const uint32_t sbits = (g_->tune.fold_owner && Lbits >= 2 && rb_ < (uint32_t)PT_MAXBITS)
                                   ? std::min<uint32_t>(Lbits - 1, (uint32_t)PT_MAXBITS - rb_)
                                   : 0u;
        const uint32_t S = 1u << sbits, FA = (uint32_t)world_ * S;

        // ---- stage A on every local rank, both sides
        struct SideX {
            Parted                A;       // partitioned by (owner rank, first local digit)
            BufP                  recv[MAX_WORDS];
            WordSrc               ws;      // what arrived
            Ev                    ready, done, counted;
            ExchangePlan          plan;
            BufP                  segs;    // device copy of plan.seg_begin | seg_end | part_off
        };
        std::vector<SideX>         bx((size_t)nl_), px((size_t)nl_);
        std::vector<Exec::CoParts> parts((size_t)nl_);  // stage B partitions of both sides
        if (((size_t)FA + 1) * 4 > Context::SMALL_PINNED / 4)
            throw_fmt(RJ_ERR_UNSUPPORTED, "sharded join: more than %zu stage-A partitions", Context::SMALL_PINNED / 16 - 1);
        for (int l = 0; l < nl_; ++l) {
            guarded(lerr[l], [&] {
                use(l);
                inject_failure(2, l);
                Exec&    E = *ex_[l];
                Context* c = g_->lane(l);
                for (int side = 0; side < 2; ++side) {
                    Exec::Side& s = side == 0 ? st[l].bs() : st[l].ps();
                    SideX&      X = side == 0 ? bx[l] : px[l];
                    TupleSrc    src = E.make_src(st[l], s, js);
                    X.ready.make();
                    X.done.make();
                    X.counted.make();
                    // the per-partition offsets leave for the host BEFORE the scatter is enqueued: the
                    // host sizes and starts the exchange of the build side while the probe side's
                    // scatter is still running
                    // (pinned block: [0, 1/4) and [1/4, 1/2) = the two sides' stage-A offsets, [1/2, 3/4) and
                    // [3/4, 1) = their exchanged-run tables, below)
                    uint32_t* host_off = static_cast<uint32_t*>(c->small_pinned()) + (size_t)side * (Context::SMALL_PINNED / 16);
                    const std::function<void(const uint32_t*)> counts_out = [&](const uint32_t* off) {
                        RJ_HIP(hipMemcpyAsync(host_off, off, ((size_t)FA + 1) * 4, hipMemcpyDeviceToHost, c->stream));
                        RJ_HIP(hipEventRecord(X.counted.e, c->stream));
                    };
                    PassShape shape;
                    if (rb_ && sbits) {
                        shape.hi_shift = 32 - rb_;
                        shape.lo_bits = sbits;
                    }
                    // one field when only one of the two digits exists: the owner's (top bits) or the local one's (low bits)
                    const uint32_t shiftA = sbits ? 0u : (rb_ ? 32 - rb_ : 31);
                    PartitionRequest rq = PartitionRequest::columns(src, KW, s.CW, rb_ + sbits);
                    rq.shift0 = shiftA;
                    rq.single_pass = true;
                    rq.after_offsets = &counts_out;
                    rq.shape = shape.hi_shift ? &shape : nullptr;
                    X.A = E.partition(rq);
                    // (test hook: this rank's probe-side slices are "never" ready — 7 s — so that the
                    // bounded wait for their exchange can be seen to expire; the counts left earlier)
                    if (g_->tune.debug_shard_fail == 4 && g_->tune.debug_shard_fail_rank == rank_base_ + l && side == 1)
                        launch_debug_stall(E.L, 7000);
                    RJ_HIP(hipEventRecord(X.ready.e, c->stream));
                }
            });
        }
        // ---- who holds how much for whom: cnt[src rank][side][dst rank][digit], + a status word
        const size_t per_side = (size_t)world_ * S;
        for (int l = 0; l < nl_; ++l) {
            mine[l].assign(2 * per_side + 1, 0);
            guarded(lerr[l], [&] {
                use(l);
                Context* c = g_->lane(l);
                for (int side = 0; side < 2; ++side) {
                    SideX& X = side == 0 ? bx[l] : px[l];
                    RJ_HIP(hipEventSynchronize(X.counted.e));  // (this rank's own stream: finite)
                    const uint32_t* off = static_cast<const uint32_t*>(c->small_pinned()) + (size_t)side * (Context::SMALL_PINNED / 16);
                    for (size_t q = 0; q < per_side; ++q) mine[l][side * per_side + q] = off[q + 1] - off[q];
                }
            });
            if (lerr[l].code) mine[l].assign(2 * per_side + 1, 0);
            mine[l][2 * per_side] = (uint64_t)lerr[l].code;
        }
        lap("stage A (histograms on the host; scatters may still run)");
        gather(mine, 2 * per_side + 1, all);
        agree(all, 2 * per_side, lerr, "partitioning its shard (stage A)");
        lap("count all-gather");

        // ---- the exchange layout (host arithmetic, rj_xplan.cpp).  Whether a rank would receive
        // more than 2^32 tuples is decided for EVERY rank of the world from the same tensor, so
        // all ranks throw the same error here — none of them enters the collective alone.
        std::vector<uint64_t> cnt[2];
        for (int side = 0; side < 2; ++side) {
            cnt[side].resize((size_t)world_ * per_side);
            for (int r = 0; r < world_; ++r)
                std::copy(all[r].begin() + side * per_side, all[r].begin() + (side + 1) * per_side,
                          cnt[side].begin() + (size_t)r * per_side);
            const int over = exchange_first_overflow((uint32_t)world_, S, cnt[side].data());
            if (over >= 0)
                throw_fmt(RJ_ERR_UNSUPPORTED, "sharded join: rank %d would receive more than 2^32 tuples of the %s side", over,
                          side == 0 ? "build" : "probe");
        }
        // receive buffers (a local allocation may fail: agreed on with one more status word)
        for (int l = 0; l < nl_; ++l) {
            guarded(lerr[l], [&] {
                use(l);
                inject_failure(3, l);
                Context* c = g_->lane(l);
                for (int side = 0; side < 2; ++side) {
                    SideX&    X = side == 0 ? bx[l] : px[l];
                    const int CW = side == 0 ? st[l].bs().CW : st[l].ps().CW;
                    exchange_plan((uint32_t)world_, S, (uint32_t)(rank_base_ + l), cnt[side].data(), X.plan);
                    X.ws.n = X.plan.n_recv;
                    X.ws.packed = X.A.packed;
                    for (int a = 0; a < MAX_WORDS; ++a) {
                        const uint32_t wbytes = array_width(X.A, KW, CW, a);
                        if (!wbytes) continue;
                        X.recv[a] = c->buf(std::max<uint64_t>(X.plan.n_recv, 1) * wbytes);
                        X.ws.w.w[a] = X.recv[a]->as<uint32_t>();
                    }
                    if (S > 1) {  // the runs that arrive, as input segments of stage B's first pass
                        // (through PINNED memory: an asynchronous copy from pageable memory makes the
                        // host wait for everything queued on the stream — stage A's scatters — and the
                        // exchange, which is to overlap them, would not even be enqueued until then)
                        const size_t ns = X.plan.seg_begin.size(), words = 2 * ns + S + 1;
                        if (words * 4 > Context::SMALL_PINNED / 4) throw_fmt(RJ_ERR_UNSUPPORTED, "sharded join: too many exchanged runs");
                        uint32_t* h = static_cast<uint32_t*>(c->small_pinned()) + Context::SMALL_PINNED / 8 + (size_t)side * (Context::SMALL_PINNED / 16);
                        std::copy(X.plan.seg_begin.begin(), X.plan.seg_begin.end(), h);
                        std::copy(X.plan.seg_end.begin(), X.plan.seg_end.end(), h + ns);
                        std::copy(X.plan.part_off.begin(), X.plan.part_off.end(), h + 2 * ns);
                        X.segs = c->buf(words * 4);
                        RJ_HIP(hipMemcpyAsync(X.segs->p, h, words * 4, hipMemcpyHostToDevice, c->stream));
                    }
                }
            });
            mine[l] = {(uint64_t)lerr[l].code};
        }
        gather(mine, 1, all);
        agree(all, 0, lerr, "allocating its receive buffers");

        // ---- the exchange: build side first, probe side queued behind it on the exchange streams
        for (int side = 0; side < 2; ++side) {
            std::vector<SideX>& XS = side == 0 ? bx : px;
            // arrays of the partition layout (the same on every rank: KW, CW and the packing rule agree)
            const int CW = side == 0 ? st[0].bs().CW : st[0].ps().CW;
            // one all-to-all per relation: every array of the layout travels in the same group
            std::vector<std::vector<XferSpec>> specs((size_t)nl_);
            std::vector<hipEvent_t>            ready, done;
            for (int l = 0; l < nl_; ++l) {
                SideX& X = XS[l];
                for (int a = 0; a < MAX_WORDS; ++a) {
                    const uint32_t wbytes = array_width(X.A, KW, CW, a);
                    if (!wbytes) continue;
                    XferSpec sp;
                    sp.send = reinterpret_cast<const uint8_t*>(X.A.w.w[a]);
                    sp.recv = reinterpret_cast<uint8_t*>(X.ws.w.w[a]);
                    for (int r = 0; r < world_; ++r) {
                        sp.send_off.push_back(X.plan.send_off[r] * wbytes);
                        sp.send_cnt.push_back(X.plan.send_cnt[r] * wbytes);
                        sp.recv_off.push_back(X.plan.recv_off[r] * wbytes);
                        sp.recv_cnt.push_back(X.plan.recv_cnt[r] * wbytes);
                    }
                    specs[l].push_back(std::move(sp));
                }
                ready.push_back(X.ready.e);
                done.push_back(X.done.e);
            }
            if (comm_) {
                comm_->all_to_all(specs, ready, done, side == 0 ? "exchange_build" : "exchange_probe");
            } else {  // one rank, no transport: the slice is the whole
                use(0);
                for (const XferSpec& sp : specs[0])
                    RJ_HIP(hipMemcpyAsync(sp.recv, sp.send, sp.send_cnt[0], hipMemcpyDeviceToDevice, g_->stream));
                RJ_HIP(hipEventRecord(done[0], g_->stream));
            }
        }

        lap("exchange (both sides)");
        // ---- stage B: each rank joins what it owns.  The host waits for an exchange with a
        // bound (Comm::wait_event) BEFORE it makes the compute stream depend on it, so no stream
        // and no host thread of this rank ever sits behind a peer that is gone.
        std::vector<Rel> out((size_t)nl_);
        auto stage_b = [&](int l, SideX& X, int CW) {
            Exec& E = *ex_[l];
            if (S == 1) return E.partition(PartitionRequest::words(X.ws, KW, CW, Lbits));
            const size_t ns = X.plan.seg_begin.size();
            PassShape    shape;
            shape.seg_begin = X.segs->as<uint32_t>();
            shape.seg_end = shape.seg_begin + ns;
            shape.oseg_off = shape.seg_begin + 2 * ns;
            shape.nseg = (uint32_t)ns;
            shape.n_oseg = S;
            shape.oseg_shift = rb_;  // `world` runs per digit
            shape.prior_bits = {sbits};
            PartitionRequest rq = PartitionRequest::words(X.ws, KW, CW, Lbits - sbits);
            rq.shift0 = sbits;
            rq.shape = &shape;
            return E.partition(rq);
        };
        // (what fails on ONE rank from here on — an allocation, a result beyond 2^32 rows — is kept and
        // reported with the next join's first status word, or at the end of the plan: the peers are
        // not in a collective with this rank any more, but would be in the next join)
        if (pending_.empty()) pending_.resize((size_t)nl_);
        for (int side = 0; side < 2; ++side)
            for (int l = 0; l < nl_; ++l) {
                SideX& X = side == 0 ? bx[l] : px[l];
                if (comm_) comm_->wait_event(l, X.done.e, side == 0 ? "the exchange of the build side" : "the exchange of the probe side");
                guarded(pending_[l], [&] {
                    use(l);
                    RJ_HIP(hipStreamWaitEvent(g_->lane(l)->stream, X.done.e, 0));
                    (side == 0 ? parts[l].B : parts[l].P) = stage_b(l, X, side == 0 ? st[l].bs().CW : st[l].ps().CW);
                });
            }
        for (int l = 0; l < nl_; ++l)
            guarded(pending_[l], [&] {
                use(l);
                inject_failure(6, l);
                st[l].cap_hint = std::max(bx[l].ws.n, px[l].ws.n);
                out[l] = ex_[l]->join_finish(st[l], js, &parts[l], Lbits, root_res ? (*root_res)[l] : nullptr);
            });
        lap("stage B (passes + join)");
        // stage A's arrays were read by the exchange streams (and by peers): they may go back
        // to the block caches only now that every rank's outgoing copies have left
        sync_all();
        for (int l = 0; l < nl_; ++l) wait_xfer(l, "the exchange streams");
        return out;
    }

    void gather(const std::vector<std::vector<uint64_t>>& mine, size_t k,
                std::vector<std::vector<uint64_t>>& all) {
        if (comm_) {
            comm_->allgather_u64(mine, k, all);
        } else {
            all.assign(1, mine[0]);
        }
    }
};

// The first node, in the order of the plan walk, of a kind that does not run sharded (found before
// any rank moves data); nullptr = none.  A malformed plan is the plan walk's to report.
const NodeKind* first_unshardable(const rj_plan* plan, uint64_t idx, int depth) {
    if (!plan || idx >= plan->n_nodes || depth > 4096) return nullptr;
    const rj_node&  n = plan->nodes[idx];
    const NodeKind* K = node_kind(n.kind);
    if (!K || !K->sharded) return K;
    const NodeKind* below = nullptr;
    if (K->children >= 1) below = first_unshardable(plan, n.left, depth + 1);
    if (!below && K->children >= 2) below = first_unshardable(plan, n.right, depth + 1);
    return below;
}
std::string one_device_only(const NodeKind& K) { return std::string(K.name) + " node (" + K.token + ") runs on one device"; }

bool node_shardable(const rj_plan* plan, uint64_t idx, int depth, std::string* why) {
    if (idx >= plan->n_nodes || depth > 4096) return false;
    const rj_node& n = plan->nodes[idx];
    if (n.kind == RJ_NODE_SCAN) {
        for (uint64_t k = 0; k < n.n_out; ++k)
            if (n.out_type[k] == RJ_VARCHAR) {
                if (why) *why = "a scan outputs a VARCHAR column";
                return false;
            }
        return true;
    }
    if (n.kind != RJ_NODE_JOIN) return false;  // (plan_shardable has named the kind: first_unshardable)
    if (!node_shardable(plan, n.left, depth + 1, why) || !node_shardable(plan, n.right, depth + 1, why))
        return false;
    if (n.left >= plan->n_nodes || n.right >= plan->n_nodes) return false;
    const uint64_t lw = plan->nodes[n.left].n_out, rw = plan->nodes[n.right].n_out;
    if (n.left_attr >= lw || n.right_attr >= rw) return false;
    // what must travel with the key on each side: up to MAX_WORDS - KW carry words (a nullable
    // column needs one word more for its validity bits — known only at run time, where the ranks
    // then agree to refuse the join together)
    const rj_node& build = n.build_left ? plan->nodes[n.left] : plan->nodes[n.right];
    const int32_t  key_type = build.out_type[n.build_left ? n.left_attr : n.right_attr];
    const int      KW = key_type == RJ_INT32 ? 1 : 2;
    std::set<uint64_t> need_l, need_r;
    for (uint64_t k = 0; k < n.n_out; ++k) {
        const uint64_t c = n.out_idx[k];
        if (c >= lw + rw) return false;
        if (c < lw) {
            if (c != n.left_attr) need_l.insert(c);
        } else if (c - lw != n.right_attr) {
            need_r.insert(c - lw);
        }
    }
    auto words = [&](const rj_node& child, const std::set<uint64_t>& need, int& n64) {
        int w = 0;
        n64 = 0;
        for (uint64_t c : need) {
            const bool wide = child.out_type[c] == RJ_INT64 || child.out_type[c] == RJ_FP64;
            w += wide ? 2 : 1;
            n64 += wide;
        }
        return w;
    };
    for (int side = 0; side < 2; ++side) {
        int       n64 = 0;
        const int w = words(side == 0 ? plan->nodes[n.left] : plan->nodes[n.right], side == 0 ? need_l : need_r, n64);
        if (w > MAX_WORDS - KW || n64 > 1 || (n64 == 1 && w == 4)) {
            if (why) *why = "a join side needs more payload than travels with the key (more than 3 carry words, or two 64-bit columns)";
            return false;
        }
    }
    return true;
}
}  // namespace

// ------------------------------------------------------------------ RJ_NODE_MAP: the program
static_assert((int)X_COL == RJ_X_COL && (int)X_NULL == RJ_X_NULL && (int)X_MOD == RJ_X_MOD && (int)X_ABS == RJ_X_ABS && (int)X_GEQ == RJ_X_GEQ &&
                  (int)X_NOT == RJ_X_NOT && (int)X_IS_NOT_NULL == RJ_X_IS_NOT_NULL && (int)X_CASE == RJ_X_CASE && (int)X_TO_F64 == RJ_X_TO_F64 &&
                  (int)X_OUT == RJ_X_OUT && MAP_MAX_OPS == RJ_MAP_MAX_OPS && MAP_MAX_DEPTH == RJ_MAP_MAX_DEPTH,
              "rj_expr.hpp mirrors rj_expr_opcode");

void map_check(const rj_expr_op* ops, uint64_t n_ops, uint64_t n_cols, const int32_t* col_type, const uint8_t* col_nullable,
               std::vector<MapOp>& dev_ops, std::vector<MapExpr>& exprs) {
    dev_ops.clear();
    exprs.clear();
    if (n_ops > (uint64_t)MAP_MAX_OPS) throw_fmt(RJ_ERR_UNSUPPORTED, "map: program longer than %d operations", MAP_MAX_OPS);
    if (n_ops && !ops) throw_fmt(RJ_ERR_ARG, "map: %llu operations but a NULL program pointer", (unsigned long long)n_ops);
    struct Slot {
        bool f64, nullable;
    };
    Slot st[MAP_MAX_DEPTH + 1];
    int  sp = 0;
    auto need = [&](int k, uint64_t at) {
        if (sp < k) throw_fmt(RJ_ERR_ARG, "map: stack underflow at op %llu", (unsigned long long)at);
    };
    auto same = [&](const Slot& x, const Slot& y, uint64_t at) {
        if (x.f64 != y.f64) throw_fmt(RJ_ERR_ARG, "map: operands of different types at op %llu (cast first)", (unsigned long long)at);
    };
    auto integer = [&](const Slot& x, uint64_t at, const char* what) {
        if (x.f64) throw_fmt(RJ_ERR_ARG, "map: %s takes integer operands (op %llu)", what, (unsigned long long)at);
    };
    for (uint64_t k = 0; k < n_ops; ++k) {
        const rj_expr_op& o = ops[k];
        MapOp             d{};
        d.op = o.op;
        Slot r{false, false};
        bool push = true;
        if (o.op == RJ_X_COL) {
            if (o.column < 0 || (uint64_t)o.column >= n_cols) throw_fmt(RJ_ERR_ARG, "map: column out of range at op %llu", (unsigned long long)k);
            const int32_t t = col_type[o.column];
            if (t == RJ_VARCHAR)
                throw_fmt(RJ_ERR_UNSUPPORTED, "map: expression over a VARCHAR column (child column %d): a VARCHAR value travels as a row "
                                              "id, its pages are not read here", o.column);
            if (t != RJ_INT32 && t != RJ_INT64 && t != RJ_FP64) throw_fmt(RJ_ERR_ARG, "map: bad column type %d", t);
            r = Slot{t == RJ_FP64, col_nullable ? col_nullable[o.column] != 0 : true};
        } else if (o.op == RJ_X_INT || o.op == RJ_X_F64) {
            d.lit = o.ivalue;
            r = Slot{o.op == RJ_X_F64, false};
        } else if (o.op == RJ_X_NULL) {
            if (o.column != RJ_INT64 && o.column != RJ_FP64)
                throw_fmt(RJ_ERR_ARG, "map: RJ_X_NULL with type code %d (RJ_INT64 or RJ_FP64)", o.column);
            r = Slot{o.column == RJ_FP64, true};
        } else if (o.op >= RJ_X_ADD && o.op <= RJ_X_MOD) {
            need(2, k);
            const Slot &a = st[sp - 2], &b = st[sp - 1];
            same(a, b, k);
            if (o.op == RJ_X_MOD && a.f64) throw_fmt(RJ_ERR_ARG, "map: MOD on F64 (op %llu)", (unsigned long long)k);
            d.arity = 2;
            d.f64 = a.f64;
            r = Slot{a.f64, a.nullable || b.nullable || (!a.f64 && (o.op == RJ_X_DIV || o.op == RJ_X_MOD))};
        } else if (o.op == RJ_X_NEG || o.op == RJ_X_ABS) {
            need(1, k);
            d.arity = 1;
            d.f64 = st[sp - 1].f64;
            r = st[sp - 1];
        } else if (o.op >= RJ_X_EQ && o.op <= RJ_X_GEQ) {
            need(2, k);
            const Slot &a = st[sp - 2], &b = st[sp - 1];
            same(a, b, k);
            d.arity = 2;
            d.f64 = a.f64;
            r = Slot{false, a.nullable || b.nullable};
        } else if (o.op == RJ_X_AND || o.op == RJ_X_OR) {
            need(2, k);
            integer(st[sp - 2], k, "AND / OR");
            integer(st[sp - 1], k, "AND / OR");
            d.arity = 2;
            r = Slot{false, st[sp - 2].nullable || st[sp - 1].nullable};
        } else if (o.op == RJ_X_NOT) {
            need(1, k);
            integer(st[sp - 1], k, "NOT");
            d.arity = 1;
            r = st[sp - 1];
        } else if (o.op == RJ_X_IS_NULL || o.op == RJ_X_IS_NOT_NULL) {
            need(1, k);
            d.arity = 1;
            d.f64 = st[sp - 1].f64;
            r = Slot{false, false};
        } else if (o.op == RJ_X_COALESCE) {
            need(2, k);
            const Slot &a = st[sp - 2], &b = st[sp - 1];
            same(a, b, k);
            d.arity = 2;
            d.f64 = a.f64;
            r = Slot{a.f64, a.nullable && b.nullable};
        } else if (o.op == RJ_X_CASE) {
            need(3, k);
            const Slot &c = st[sp - 3], &a = st[sp - 2], &b = st[sp - 1];
            integer(c, k, "the condition of CASE");
            same(a, b, k);
            d.arity = 3;
            d.f64 = a.f64;
            r = Slot{a.f64, a.nullable || b.nullable};
        } else if (o.op == RJ_X_TO_I64 || o.op == RJ_X_TO_F64) {
            need(1, k);
            const Slot& a = st[sp - 1];
            d.arity = 1;
            d.f64 = a.f64;
            r = Slot{o.op == RJ_X_TO_F64, a.nullable || (o.op == RJ_X_TO_I64 && a.f64)};
        } else if (o.op == RJ_X_OUT) {
            need(1, k);
            if (sp != 1) throw_fmt(RJ_ERR_ARG, "map: %d values left on the stack behind RJ_X_OUT (op %llu)", sp - 1, (unsigned long long)k);
            d.arity = 1;
            d.f64 = st[0].f64;
            exprs.push_back(MapExpr{st[0].f64 ? 1 : 0, st[0].nullable});
            push = false;
        } else {
            throw_fmt(RJ_ERR_ARG, "map: bad expression opcode %d (op %llu)", o.op, (unsigned long long)k);
        }
        sp -= d.arity;
        if (push) {
            if (sp >= MAP_MAX_DEPTH) throw_fmt(RJ_ERR_UNSUPPORTED, "map: stack deeper than %d (op %llu)", MAP_MAX_DEPTH, (unsigned long long)k);
            if (d.arity == 0) d.f64 = r.f64;
            st[sp++] = r;
        }
        dev_ops.push_back(d);
    }
    if (sp != 0) throw_fmt(RJ_ERR_ARG, "map: the program does not end in RJ_X_OUT (%d values left on the stack)", sp);
}

void map_eval_row(const rj_expr_op* ops, uint64_t n_ops, uint64_t n_cols, const int32_t* col_type, const uint64_t* col_bits,
                  const uint8_t* col_null, uint64_t out_cap, uint64_t* out_bits, uint8_t* out_null, int32_t* out_kind, uint64_t* n_out) {
    std::vector<MapOp>   dev;
    std::vector<MapExpr> exprs;
    map_check(ops, n_ops, n_cols, col_type, nullptr, dev, exprs);
    uint64_t v[MAP_MAX_DEPTH + 3] = {};
    bool     nl[MAP_MAX_DEPTH + 3] = {};
    uint32_t sp = 0;
    uint64_t e = 0;
    for (uint64_t k = 0; k < n_ops; ++k) {
        const MapOp& o = dev[k];
        uint64_t     r = 0;
        bool         rn = false;
        if (o.op == X_COL) {
            const int32_t c = ops[k].column;
            r = col_type[c] == RJ_INT32 ? (uint64_t)(int64_t)(int32_t)(uint32_t)col_bits[c] : col_bits[c];
            rn = col_null[c] != 0;
        } else if (o.op <= X_NULL) {
            r = (uint64_t)o.lit;
            rn = o.op == X_NULL;
        } else {
            const uint32_t base = sp - (uint32_t)o.arity;
            if (o.op == X_OUT) {
                if (e < out_cap) {
                    out_null[e] = nl[base] ? 1 : 0;
                    out_bits[e] = nl[base] ? 0 : x_out(o.f64 != 0, v[base]);
                    out_kind[e] = o.f64 ? RJ_FP64 : RJ_INT64;
                }
                ++e;
                sp = base;
                continue;
            }
            r = x_apply(o.op, o.f64 != 0, v[base], nl[base], o.arity >= 2 ? v[base + 1] : 0, o.arity >= 2 && nl[base + 1],
                        o.arity >= 3 ? v[base + 2] : 0, o.arity >= 3 && nl[base + 2], rn);
            sp = base;
        }
        v[sp] = r;
        nl[sp] = rn;
        ++sp;
    }
    *n_out = e;
}

Result* execute_plan(Context* ctx, const rj_plan* plan, Table* const* tables, uint64_t n_tables,
                     int flags, TableFetch* fetch) {
    Exec e(ctx, plan, tables, n_tables, flags);
    e.set_fetch(fetch);
    return e.run();
}

Result* join_tuples(Context* ctx, const rj_tuples* build, const rj_tuples* probe,
                    uint32_t skip_rank_bits, int flags) {
    Exec e(ctx, nullptr, nullptr, 0, flags);
    return e.run_tuples(build, probe, skip_rank_bits);
}

void execute_sharded(Context* group, const rj_plan* plan, Table* const* tables, uint64_t n_inputs,
                     int flags, Result** out) {
    if (const NodeKind* K = plan ? first_unshardable(plan, plan->root, 0) : nullptr)
        throw_fmt(RJ_ERR_UNSUPPORTED, "rj_execute_sharded: %s", one_device_only(*K).c_str());
    ShardedExec e(group, plan, tables, n_inputs, flags);
    e.run(out);
}

bool plan_shardable(const rj_plan* plan, std::string* why) {
    if (!plan || plan->root >= plan->n_nodes) return false;
    if (const NodeKind* K = first_unshardable(plan, plan->root, 0)) {
        if (why) *why = one_device_only(*K);
        return false;
    }
    return node_shardable(plan, plan->root, 0, why);
}

void shard_partition(Context* ctx, const Table* t, uint64_t key_col, uint64_t carry_col,
                     uint32_t n_ranks, rj_tuples* out, uint64_t* counts) {
    Exec e(ctx, nullptr, nullptr, 0, 0);
    e.run_shard(t, key_col, carry_col, n_ranks, out, counts);
}

}  // namespace rj
