/*
 * rj.h — C-ABI of the MI355X radix-join executor (librj.so).
 *
 * This is the drop-in boundary for the reference's hot path: everything the
 * reference does inside
 *
 *     namespace Contest { void* build_context(); void destroy_context(void*);
 *                         ColumnarTable execute(const Plan&, void*); }
 *     (reference include/plan.h:337-344, definitions src/execute.cpp:316-330)
 *
 * is reachable through the plain-C entry points below.  Signatures carry only
 * plain pointers and sizes (no C++/torch types).  The C++ shim that sits
 * between `Contest::execute` and this ABI is radix-join_amd/host/contest_execute.cpp;
 * the binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * All functions returning `int` return RJ_OK (0) on success and a non-zero
 * rj_status on failure; rj_last_error() then holds a message.  This mirrors
 * the reference's error behaviour (C++ exceptions derived from std::exception,
 * src/execute.cpp:280, build_table.cpp:335) — the shim rethrows
 * std::runtime_error(rj_last_error()).
 */
#ifndef RJ_H_
#define RJ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RJ_PAGE_SIZE 8192u /* reference include/plan.h:54 (PAGE_SIZE) */

/* DataType — values fixed by reference include/attribute.h:8-13 */
typedef enum rj_dtype {
    RJ_INT32   = 0,
    RJ_INT64   = 1,
    RJ_FP64    = 2,
    RJ_VARCHAR = 3
} rj_dtype;

typedef enum rj_status {
    RJ_OK            = 0,
    RJ_ERR_ARG       = 1, /* malformed plan / bad argument                    */
    RJ_ERR_DEVICE    = 2, /* HIP runtime error                                */
    RJ_ERR_NOMEM     = 3, /* device or host allocation failed                 */
    RJ_ERR_DATA      = 4, /* pages inconsistent with num_rows ("row_idx",
                             reference build_table.cpp:334-336)               */
    RJ_ERR_UNSUPPORTED = 5, /* e.g. more than 2^32 rows in one relation, a plan
                             rj_execute_sharded cannot shard                  */
    RJ_ERR_NO_GPU    = 6  /* no usable HIP device: the product path has no
                             CPU fallback and fails loudly                    */
} rj_status;

/* ------------------------------------------------------------------ plan --
 * POD flattening of reference `Plan` (include/plan.h:32-52,112-149).
 * nodes[i].kind: RJ_NODE_SCAN ↔ ScanNode{base_table_id},
 *                RJ_NODE_JOIN ↔ JoinNode{build_left,left,right,left_attr,right_attr}.
 * out_idx/out_type ↔ PlanNode::output_attrs (vector<tuple<size_t,DataType>>):
 *   scan: index into the base table's columns;
 *   join: index into concat(left child outputs, right child outputs)
 *         (reference README.md:55, src/execute.cpp:236-242).
 *
 * Semi and anti joins (no reference counterpart: WHERE EXISTS / NOT EXISTS / IN).
 * RJ_NODE_SEMI / RJ_NODE_ANTI use the fields of a join with the same meaning:
 *   build_left picks the FILTER side (the side that is built, as for RJ_NODE_JOIN); the other
 *   child is the PRESERVED side, which is probed.  out_idx indexes concat(left outputs, right
 *   outputs) as for a join and may name columns of the preserved side only (a filter-side
 *   column is RJ_ERR_ARG).
 *   SEMI: every preserved row whose key equals at least one filter-side key, once, however many
 *         partners it has.
 *   ANTI: every preserved row for which no filter-side key is equal — NOT EXISTS, not NOT IN:
 *         rows with a NULL key and FP64 rows with a NaN key are in the result, and a NULL on
 *         the filter side changes nothing.
 *   Key equality is the inner join's: the key type is the filter side's key type; INT32 / INT64
 *   compare by value; FP64 by bit pattern, a NaN matches nothing; a preserved key of another
 *   type matches nothing (SEMI: 0 rows, ANTI: every preserved row).  An empty filter side gives
 *   0 rows (SEMI) or every preserved row (ANTI); an empty preserved side 0 rows with the declared
 *   column types and zero pages.  The result is a multiset of preserved rows in no particular
 *   order.  VARCHAR keys are RJ_ERR_UNSUPPORTED; VARCHAR payload columns of the preserved side
 *   are fine.  The kinds nest freely with joins and with each other.  rj_execute_sharded refuses
 *   plans that hold them (RJ_ERR_UNSUPPORTED), rj_plan_shardable reports them, and rj_execute on
 *   a multi-device context runs such a plan on its first device.  A library older than these
 *   kinds rejects them with RJ_ERR_ARG ("bad node kind").
 *
 * Outer joins (LEFT / RIGHT OUTER JOIN; no reference counterpart).
 * RJ_NODE_OUTER uses the fields of a join with the same meaning:
 *   build_left picks the OPTIONAL side: the side that is built, and whose columns are NULL in the
 *   rows of preserved rows without a partner.  The other child is the PRESERVED side, which is
 *   probed.  SQL `left LEFT JOIN right` is build_left = 0, `left RIGHT JOIN right` build_left = 1.
 *   out_idx indexes concat(left outputs, right outputs) as for a join and may name columns of both
 *   sides, in any order, repeated or not, possibly none of one side.
 *   Result: the inner join's rows (same key rules, duplicates multiply on both sides) plus, for
 *   every preserved row that has NO partner, exactly one row holding that row's preserved columns
 *   and NULL in every optional-side column.  "No partner" is what ANTI means by it: the preserved
 *   key is NULL, is an FP64 NaN, is of another type than the optional side's key (then EVERY
 *   preserved row is unmatched), or equals no optional key.  NULL and NaN keys on the optional
 *   side match nothing and add no rows.  Key equality is the inner join's: the key type is the
 *   optional (build) side's; INT32 / INT64 compare by value, FP64 by bit pattern.
 *   The preserved side's key column, when output, is that row's own key, NULL included; the
 *   optional side's key column, when output, is NULL in unmatched rows.  An empty optional side
 *   gives every preserved row, padded; an empty preserved side 0 rows with the declared column
 *   types and zero pages.  The result is a multiset in no particular order.  An output column
 *   keeps its declared type; optional-side columns of the result are nullable even when the
 *   source column is not.
 *   VARCHAR keys are RJ_ERR_UNSUPPORTED.  VARCHAR payload columns of the preserved side are fine;
 *   a VARCHAR column of the OPTIONAL side in out_idx is RJ_ERR_UNSUPPORTED (a VARCHAR value
 *   travels as a row id of its base table, which has no way to say NULL).
 *   The kind nests freely under and over joins, semi / anti joins and other outer joins; a parent
 *   may join on a nullable column an outer join produced (NULL keys drop out as always).
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.
 *   A library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Full outer joins (FULL OUTER JOIN; no reference counterpart).
 * RJ_NODE_FULL uses the fields of a join:
 *   build_left picks which child is BUILT; the other child is PROBED.  It is an execution hint
 *   only: the result is the same multiset either way (the executor builds an empty child whatever
 *   the hint says).  out_idx indexes concat(left outputs, right outputs) and may name columns of
 *   both sides, in any order, repeated or not, possibly none of one side.
 *   Result: the union of (1) the inner join's rows (same key rules: the key type is the built
 *   side's; INT32 / INT64 compare by value, FP64 by bit pattern; NULL and NaN match nothing;
 *   duplicates multiply on both sides), (2) for every row of the probed child without a partner,
 *   one row with that child's columns and NULL in every column of the built child, and (3) for
 *   every row of the built child without a partner, one row with that child's columns and NULL in
 *   every column of the probed child.  "Without a partner" is what ANTI and OUTER mean by it, on
 *   both sides: the key is NULL, is an FP64 NaN, or equals no key of the other side; when the two
 *   key columns have different types, every row of both children is unmatched.
 *   A key column that is output is the key of the side it belongs to: that row's own key, NULL
 *   included, and NULL in the rows padded on that side.  There is no COALESCE column.
 *   An empty child gives every row of the other child, padded; two empty children give 0 rows with
 *   the declared column types and zero pages.  The result is a multiset in no particular order.
 *   Every output column keeps its declared type and is nullable, whatever the source column is.
 *   VARCHAR keys (on either side) are RJ_ERR_UNSUPPORTED, and so is a VARCHAR column of EITHER
 *   side in out_idx (both sides are optional: see RJ_NODE_OUTER).  Malformed nodes are RJ_ERR_ARG.
 *   The kind nests freely under and over joins, semi / anti joins, outer joins and itself; a
 *   parent may join on a nullable column it produced (NULL keys drop out as always).
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.
 *   A library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Aggregation (GROUP BY key with COUNT / SUM / MIN / MAX; no reference counterpart).
 * RJ_NODE_AGG has ONE child, `left`; `right`, `right_attr` and `build_left` are ignored.  left_attr
 *   is the child column that is grouped by.  Every output names an aggregate function and a child
 *   column: out_idx[k] = RJ_AGG_OUT(func, column), out_type[k] = the declared RESULT type:
 *     RJ_AGG_KEY        the group's key; column must be left_attr; the key's type; may appear 0, 1
 *                       or several times
 *     RJ_AGG_COUNT_STAR rows of the group; column must be 0; INT64
 *     RJ_AGG_COUNT      non-NULL values of an INT32 / INT64 column; INT64
 *     RJ_AGG_SUM        sum of the non-NULL values of an INT32 / INT64 column, wrapping modulo
 *                       2^64; INT64; NULL if the group has no non-NULL value
 *     RJ_AGG_MIN / RJ_AGG_MAX  over the non-NULL values of an INT32 / INT64 column; the column's
 *                       type; NULL if the group has no non-NULL value
 *   (the other kinds keep rejecting such out_idx values as out of range).
 *   Result: one row per distinct key value of the child, in no particular order.  Rows whose key is
 *   NULL form ONE group, whose key comes out NULL: SQL's GROUP BY, not the join's "NULL matches
 *   nothing".  An empty child gives 0 rows with the declared column types and zero pages.
 *   RJ_ERR_ARG: a declared type other than the table above says, an unknown function code, a
 *   column out of range, RJ_AGG_KEY on another column than left_attr, RJ_AGG_COUNT_STAR with a
 *   column, RJ_AGG_FSUM (the exact FP64 sum is RJ_NODE_GROUP's).  Key types are INT32 and INT64; FP64 and VARCHAR keys are RJ_ERR_UNSUPPORTED, and so are
 *   FP64 and VARCHAR aggregated columns (a floating-point sum depends on the order of the rows,
 *   which no result of this library does).  The child may carry columns of any type that the node
 *   does not name.  Several functions over the same column cost one carried column.
 *   Carry limit: the DISTINCT aggregated columns travel with the key through the radix passes, plus
 *   one word of validity bits if any of them is nullable: at most 3 words behind an INT32 key (three
 *   INT32 columns; an INT64 and an INT32 one; two nullable INT32 ones; one nullable INT64 one; ...)
 *   and 2 behind an INT64 key, and at most one 64-bit column next to another word.  A node that
 *   needs more is RJ_ERR_UNSUPPORTED (the message states the limit): a row-index fallback that
 *   gathers the columns per partition is deliberately not part of this kind, and neither is a
 *   scalar aggregate without a key.
 *   The node's result is an ordinary relation: the child may be any node, and a parent JOIN / SEMI /
 *   ANTI / OUTER / FULL / AGG may use every column of it, as a key too (NULL keys drop out in joins
 *   as always); the node may be the root.  rj_execute_sharded refuses plans that hold the kind
 *   (RJ_ERR_UNSUPPORTED), rj_plan_shardable reports it, and rj_execute on a multi-device context
 *   runs such a plan on its first device.  A library older than this kind rejects it with
 *   RJ_ERR_ARG ("bad node kind").
 *
 * Selection (WHERE / HAVING / projection over any relation; no reference counterpart).
 * RJ_NODE_SELECT has ONE child, `left`; `build_left`, `base_table_id` and `left_attr` are ignored.
 *   out_idx / out_type work as a scan's do, with the child's output columns in place of the base
 *   table's: entries index the child's outputs, in any order, repeated or not; a declared type that
 *   differs from the child column's is RJ_ERR_ARG; a VARCHAR child column passes through as row ids,
 *   as through a join.
 *   The predicate is a postfix program of rj_filter_op (below, at rj_table_from_csv).  rj_node cannot
 *   grow, so two of its integer fields carry the program: `right` = the number of ops, `right_attr` =
 *   (uint64_t)(uintptr_t) of a `const rj_filter_op*` that stays valid during the call — read them with
 *   RJ_SELECT_N_OPS(node) / RJ_SELECT_OPS(node).  rj_filter_op::column indexes the CHILD's outputs; a
 *   predicate column need not be an output column.  right == 0 keeps every row (a pure projection;
 *   the pointer may then be NULL).
 *   Semantics: exactly those of rj_table_from_csv's filter (see there: a comparison is false on NULL,
 *   RJ_F_NOT flips the bit, an INT32 column compares with (int32_t)ivalue, an FP64 column IEEE-wise
 *   with the double whose bits are ivalue), with RJ_F_IS_NULL / RJ_F_IS_NOT_NULL on INT32, INT64 and
 *   FP64 columns, plus the column comparisons RJ_F_COL_EQ .. RJ_F_COL_GEQ, which only this node takes.
 *   Result: the multiset of child rows for which the program leaves 1, in no particular order; a
 *   column's nullability is the child column's.  An empty child, or a predicate that keeps nothing,
 *   gives 0 rows with the declared column types and zero pages.
 *   RJ_ERR_UNSUPPORTED: any leaf on a VARCHAR column (comparison, column comparison, LIKE, IS NULL:
 *   a VARCHAR value travels as a row id, its pages are not read here); more than 64 ops.
 *   RJ_ERR_ARG: RJ_F_HOST_BITMAP (the rows of an intermediate relation have no numbering a caller
 *   could see); a column out of range; a column comparison of two different types; LIKE on a
 *   fixed-width column; an unknown opcode; a malformed program (the stack depth is at least 1 after
 *   every op, at most 60 — which the 64-op limit keeps below 33 anyway —, and exactly 1 at the end); right != 0 with a NULL pointer.  The node is
 *   checked before its child's rows are looked at: an empty child does not hide an error.
 *   The node's result is an ordinary relation: the child may be any node, a parent of any kind may use
 *   every column of it, as a key too, and the node may be the root.  rj_execute_sharded refuses plans
 *   that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable reports it, and rj_execute on a
 *   multi-device context runs such a plan on its first device.  A library older than this kind
 *   rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Sort (ORDER BY ... [LIMIT n [OFFSET m]] over any relation; no reference counterpart).
 * RJ_NODE_SORT has ONE child, `left`; `build_left` is ignored.
 *   out_idx / out_type work exactly as RJ_NODE_SELECT's: entries index the child's outputs, in any
 *   order, repeated or not; a declared type that differs from the child column's is RJ_ERR_ARG; a
 *   VARCHAR child column passes through as row ids.
 *   rj_node cannot grow, so its integer fields carry the rest — read them with the macros below:
 *   RJ_SORT_N_KEYS(node) = `right`, RJ_SORT_KEYS(node) = `right_attr` as a `const rj_sort_key*` that
 *   stays valid during the call, RJ_SORT_LIMIT(node) = `left_attr` (RJ_SORT_NO_LIMIT = UINT64_MAX: no
 *   LIMIT), RJ_SORT_OFFSET(node) = `base_table_id`.  rj_sort_key::column indexes the CHILD's outputs;
 *   a key column need not be an output column and may repeat.  rj_sort_key::flags is a set of
 *   RJ_SORT_DESC and RJ_SORT_NULLS_FIRST; the default is ascending with NULLs last, and where NULLs go
 *   does not depend on the direction.
 *   Semantics: the child's rows ordered lexicographically by the keys, the first key most
 *   significant.  INT32 / INT64 compare by value.  FP64 compares numerically by PostgreSQL's rules:
 *   -0.0 and +0.0 are equal; every NaN (any sign, any payload) equals every other NaN and is greater
 *   than +inf.  Only the comparison canonicalises: a value that is output keeps its own bits.
 *   Result: rows [offset, offset + limit) of that order (offset + limit does not overflow: it
 *   saturates); offset >= the child's rows, or limit == 0, gives 0 rows with the declared column
 *   types and zero pages, as an empty child does.  n_keys == 0 is a plain LIMIT / OFFSET over the
 *   child's row order.  A column's nullability is the child column's.
 *   Ties: the sort is stable with respect to the order the child's rows have on the device.  For a
 *   SCAN child that is the table's row order, so the result order is fully determined.  For any other
 *   child the order within a group of equal keys is unspecified, and so is which members of a tie
 *   group a LIMIT / OFFSET boundary keeps.
 *   The row order of the result is promised ONLY when the node is the plan's root (for every column
 *   type, VARCHAR and nullable columns included).  Below another node the result is an ordinary
 *   relation, the multiset of the slice (top-k in a subquery); a non-root node with neither limit
 *   nor offset changes nothing and, once validated, passes its child through.
 *   RJ_ERR_ARG: a key column or output column out of range; flag bits other than the two defined
 *   ones; n_keys != 0 with a NULL pointer; a declared-type mismatch.  RJ_ERR_UNSUPPORTED: a VARCHAR
 *   key column (it travels as a row id); more than RJ_SORT_MAX_KEYS keys; more than 2^32 - 16 child
 *   rows.  The node is checked before its child's rows are looked at: an empty child does not hide
 *   an error.
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.  A
 *   library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Grouping (GROUP BY any keys, or none, with COUNT / SUM / MIN / MAX; SELECT DISTINCT; no reference
 * counterpart).
 * RJ_NODE_GROUP has ONE child, `left`; `build_left`, `base_table_id` and `left_attr` are ignored.
 *   It is the general form of RJ_NODE_AGG: any number of keys of INT32, INT64 or FP64, any number of
 *   aggregated columns, FP64 columns under MIN / MAX / COUNT, and the aggregate without a key.  It
 *   sorts where RJ_NODE_AGG hashes, so for ONE INT32 / INT64 key and columns within that kind's carry
 *   limit RJ_NODE_AGG is the faster node (DESIGN.md §4 has the figures).
 *   Keys: rj_node cannot grow, so RJ_GROUP_N_KEYS(node) = `right` (0 .. RJ_SORT_MAX_KEYS) and
 *   RJ_GROUP_KEYS(node) = `right_attr` as a `const rj_sort_key*` that stays valid during the call.
 *   rj_sort_key::column indexes the CHILD's outputs and may repeat; rj_sort_key::flags is a set of
 *   RJ_SORT_DESC and RJ_SORT_NULLS_FIRST and says where the key's groups go in the result's order.
 *   Outputs: as for RJ_NODE_AGG, out_idx[k] = RJ_AGG_OUT(func, column), out_type[k] = the declared
 *   RESULT type; any number of outputs over any number of distinct columns:
 *     RJ_AGG_KEY        the group's value of a key column; column must be one of the key columns;
 *                       that column's type; a key may appear 0, 1 or several times
 *     RJ_AGG_COUNT_STAR rows of the group; column must be 0; INT64
 *     RJ_AGG_COUNT      non-NULL values of an INT32 / INT64 / FP64 column; INT64
 *     RJ_AGG_SUM        sum of the non-NULL values of an INT32 / INT64 column, wrapping modulo 2^64;
 *                       INT64; NULL if the group has no non-NULL value
 *     RJ_AGG_MIN / RJ_AGG_MAX  over the non-NULL values of an INT32 / INT64 / FP64 column; the
 *                       column's type; NULL if the group has no non-NULL value
 *     RJ_AGG_FSUM       the exactly rounded sum of the non-NULL values of an FP64 column; FP64; NULL
 *                       if the group has no non-NULL value (the count decides, never a sentinel);
 *                       nullable when the child column is, or the child is empty, as RJ_AGG_SUM
 *   RJ_AGG_FSUM, for every group and for the scalar aggregate: any NaN among the values, or +inf and
 *   -inf together, give 0x7ff8000000000000.  Only +inf among the infinities gives +inf, only -inf
 *   gives -inf, whatever the finite values are.  Otherwise the result is S, the exact real sum of the
 *   finite values, rounded to nearest, ties to even, ONCE — what math.fsum returns.  |S| that rounds
 *   to 2^1024 or more gives +-inf; there is no intermediate overflow (1e308 + 1e308 - 1e308 - 1e308
 *   + 1.0 is 1.0); results in the subnormal range are exact, every double being a multiple of
 *   2^-1074.  S = 0 gives +0.0, also when every value is -0.0: the canonical zero of this node's keys
 *   and MIN / MAX.  The value depends only on the multiset of the child's rows: not on their order
 *   on the device, not on how the inputs are cut into pages, not on RJ_TUNE_GROUP_GRID.  It may stand
 *   next to KEY / COUNT(*) / COUNT / MIN / MAX over the same or other columns, in any order, repeated.
 *   AVG is not a function of its own: an RJ_NODE_MAP above the node computes
 *   FSUM(x) / TO_F64(COUNT(x)), which is NULL where the group has no value and rounds a second time.
 *   Grouping equality: two rows are in one group exactly when they tie on every key under
 *   rj_debug_sort_key's encoding.  So a NULL equals a NULL, per column — (NULL, 1), (1, NULL) and
 *   (NULL, NULL) are three groups —, -0.0 equals +0.0 and every NaN equals every other NaN.
 *   Values: a key column holds the group's CANONICAL value, the decoding of the encoded key
 *   (rj_debug_sort_key_value): the value itself for INT32 / INT64, +0.0 for either zero,
 *   0x7ff8000000000000 for any NaN, NULL for the NULL group.  FP64 MIN / MAX order by the same
 *   encoding — a NaN is above +inf — and return the canonical value too.  The result is therefore
 *   one deterministic multiset whatever order the child's rows have.
 *   Rows: one per group.  n_keys == 0 is the scalar aggregate, ONE group of all rows: over an empty
 *   child it gives ONE row, the counts 0 and SUM / MIN / MAX NULL, as SQL does.  With keys an empty
 *   child gives 0 rows with the declared column types and zero pages.  A node without any aggregate
 *   is SELECT DISTINCT.
 *   Order: the groups come out ordered by the keys under their flags, the first key most
 *   significant, as RJ_NODE_SORT orders rows.  As for that kind the order is promised ONLY when the
 *   node is the plan's root; below another node the result is an ordinary relation, and a parent of
 *   any kind may use every column of it, as a key too.
 *   RJ_ERR_ARG: a key column or output column out of range; flag bits other than the two defined
 *   ones; n_keys != 0 with a NULL pointer; an unknown function code; RJ_AGG_KEY on a column that is
 *   not a key; RJ_AGG_COUNT_STAR with a column; a declared type other than the table above says;
 *   RJ_AGG_FSUM on an INT32 / INT64 column (RJ_AGG_SUM is the integer sum).
 *   RJ_ERR_UNSUPPORTED: a VARCHAR key; a VARCHAR aggregated column (it travels as a row id, so
 *   MIN(title) is out of scope); RJ_AGG_SUM over an FP64 column (a wrapping sum has no meaning there
 *   and a sum of rounded additions depends on the order of the rows, which no result of this library
 *   does: RJ_AGG_FSUM is the FP64 sum); more than RJ_SORT_MAX_KEYS keys; more than 2^32 - 16 child rows.
 *   The child may carry VARCHAR columns that the node does not name.  The node is checked before
 *   its child's rows are looked at: an empty child does not hide an error.
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.  A
 *   library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Window functions (ROW_NUMBER / RANK / DENSE_RANK and COUNT / SUM / MIN / MAX ... OVER (PARTITION BY
 * ... ORDER BY ...); no reference counterpart).
 * RJ_NODE_WINDOW has ONE child, `left`; `build_left` is ignored, and so is `base_table_id` unless an
 * output's function is RJ_WIN_LAG or above (the section behind this one).
 *   Keys: rj_node cannot grow, so RJ_WINDOW_N_KEYS(node) = `right` is the total number of keys
 *   (0 .. RJ_SORT_MAX_KEYS), RJ_WINDOW_KEYS(node) = `right_attr` a `const rj_sort_key*` that stays
 *   valid during the call, and RJ_WINDOW_N_PART(node) = `left_attr` says how many of them, the first
 *   ones, are PARTITION BY keys; the rest are ORDER BY keys.  rj_sort_key::column indexes the CHILD's
 *   outputs and may repeat, in one list or in both.
 *   Outputs: out_idx[k] = RJ_WIN_OUT(func, column) (the bit layout of RJ_AGG_OUT), out_type[k] = the
 *   declared RESULT type; any number of outputs over any number of distinct columns:
 *     RJ_WIN_COL         a child column passes through: out_idx[k] is then a plain column index, as a
 *                        selection's; the child column's type, bits and nullability; a VARCHAR column
 *                        passes through as row ids
 *     RJ_WIN_ROW_NUMBER  1 + the rows of the partition in front of this one in the sorted order
 *     RJ_WIN_RANK        1 + the rows of the partition in front of this row's first peer
 *     RJ_WIN_DENSE_RANK  the number of peer groups of the partition up to and including this row's
 *                        (these three: column must be 0; INT64; never NULL)
 *     RJ_WIN_COUNT_STAR  rows of the frame; column must be 0; INT64
 *     RJ_WIN_COUNT       non-NULL values of an INT32 / INT64 / FP64 column in the frame; INT64
 *     RJ_WIN_SUM         sum of the non-NULL values of an INT32 / INT64 column in the frame, wrapping
 *                        modulo 2^64; INT64; NULL if the frame has no non-NULL value
 *     RJ_WIN_MIN / RJ_WIN_MAX  over the non-NULL values of an INT32 / INT64 / FP64 column in the frame;
 *                        the column's type; NULL if the frame has none
 *   Equality and order: two rows are in one partition exactly when they tie on every partition key
 *   under rj_debug_sort_key's encoding — the grouping equalities of RJ_NODE_GROUP: NULL = NULL per
 *   column, -0.0 = +0.0, NaN = NaN.  Inside a partition the rows are ordered by the order keys under
 *   their flags, as RJ_NODE_SORT orders them.  Two rows of a partition are PEERS when they tie on
 *   every order key; with no order key all rows of a partition are peers.  The flags of a partition
 *   key only say where its partitions go in the result's order.
 *   Frame: SQL's default and no other.  With order keys it is RANGE BETWEEN UNBOUNDED PRECEDING AND
 *   CURRENT ROW: every row of the partition up to and INCLUDING the current row's last peer.  Without
 *   order keys it is the whole partition.  Every aggregate value therefore depends only on the
 *   multiset of child rows, never on their order on the device.  A result is NULL where the frame
 *   has no non-NULL value, which the count decides, never a sentinel.  FP64 MIN / MAX order by the
 *   sort encoding — a NaN is above +inf — and return the canonical value (rj_debug_sort_key_value),
 *   as RJ_NODE_GROUP does.
 *   Rows: exactly the child's rows, each once, ordered by (partition keys, order keys), the first key
 *   most significant.  As for RJ_NODE_SORT and RJ_NODE_GROUP the order is promised ONLY when the node
 *   is the plan's root.  Ties are stable with respect to the child's order on the device: for a
 *   SCAN child ROW_NUMBER among peers and the result order are fully determined, for any other child
 *   which peer gets which row number is unspecified.  An empty child gives 0 rows with the declared
 *   types and zero pages.  With no key at all there is one partition of all rows, in the child's
 *   order, and nothing is sorted.
 *   RJ_ERR_ARG: n_part > n_keys; a key or output column out of range; flag bits other than the two
 *   defined ones; n_keys != 0 with a NULL pointer; a function code that rj_win_func does not define; a ranking
 *   function or RJ_WIN_COUNT_STAR with a column other than 0; a declared type other than the table
 *   above says (for RJ_WIN_COL the child column's type).
 *   RJ_ERR_UNSUPPORTED: a VARCHAR key; a VARCHAR column under a function (it travels as a row id);
 *   SUM over an FP64 column (it depends on the order of the rows); more than RJ_SORT_MAX_KEYS keys in
 *   total; more than 2^32 - 16 child rows.  The node is checked before its child's rows are looked
 *   at: an empty child does not hide an error.
 *   Out of scope: RANGE and GROUPS frames with offsets; EXCLUDE; NTH_VALUE; IGNORE NULLS; a default
 *   for LAG / LEAD; VARCHAR anywhere but passing through; sharding.
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.  A
 *   library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * ROWS frames and LAG / LEAD / FIRST_VALUE / NTILE (further functions of RJ_NODE_WINDOW; no reference
 * counterpart).  One node may hold any mix of the functions above and of these; everything the
 * section above says about keys, partitions, the order of the result and sharding holds unchanged.
 *   Arguments: rj_node cannot grow, so RJ_WINDOW_ARGS(node) = `base_table_id` is a `const rj_win_arg*`
 *   to n_out entries, entry k for output k, valid during the call.  It is read ONLY when some output's
 *   function is RJ_WIN_LAG or above, and then only the entries of those outputs; for every other plan
 *   the field stays ignored.  The same (function, column) may appear several times with different
 *   arguments, each an output of its own.
 *   Positions: position i = 0, 1, ... counts the rows in the node's order — by (partition keys,
 *   order keys), ties stable with respect to the child's order on the device.  The row at position i
 *   lies in the partition [ps, pe].  As for ROW_NUMBER, a result that depends on the order among
 *   peers (every function of this section can) is fully determined over a SCAN child and unspecified
 *   among peers over any other child.
 *   Frame: ROWS BETWEEN lo AND hi, both as SIGNED OFFSETS from the current row: negative = PRECEDING,
 *   0 = CURRENT ROW, positive = FOLLOWING, RJ_WIN_UNBOUNDED_PRECEDING (INT64_MIN) and
 *   RJ_WIN_UNBOUNDED_FOLLOWING (INT64_MAX).  The frame of position i is the positions [a, b] with
 *   a = max(ps, i + lo) and b = min(pe, i + hi); it is EMPTY when a > b (ROWS BETWEEN 3 PRECEDING AND
 *   1 PRECEDING at a partition's first row).  No offset overflows: any offset beyond +-2^32 acts as
 *   unbounded, a relation having fewer than 2^32 - 16 rows (rj_debug_win_frame is this arithmetic).
 *   A frame never leaves the partition and never looks at peers: it counts rows.
 *     RJ_WIN_LAG / RJ_WIN_LEAD  arg.lo = k >= 0, arg.hi = 0: the value of the column at position i - k
 *                        (LAG) or i + k (LEAD) if that lies in [ps, pe], else NULL; k = 0 is the row
 *                        itself and any k up to INT64_MAX is legal.  The column's type, the value's own
 *                        bits (nothing is canonicalised), always nullable.  There is no default argument:
 *                        an RJ_X_COALESCE in a MAP above supplies one, and a NULL source value and a
 *                        missing row then look alike.
 *     RJ_WIN_FIRST_VALUE / RJ_WIN_LAST_VALUE  arg = the frame: the value of the column at a / at b; NULL
 *                        if the frame is empty or that value is NULL.  The column's type, the value's own
 *                        bits, always nullable.
 *     RJ_WIN_NTILE       column must be 0, arg.lo = n >= 1, arg.hi = 0; INT64, never NULL.  PostgreSQL's
 *                        rule: with N = pe - ps + 1 rows in the partition, r = i - ps, q = N / n and
 *                        m = N % n the first m buckets hold q + 1 rows and the rest q, so the bucket is
 *                        r / (q + 1) + 1 for r < m (q + 1) and m + (r - m (q + 1)) / q + 1 otherwise;
 *                        n > N gives the buckets 1 .. N (rj_debug_win_ntile is this arithmetic).
 *     RJ_WIN_ROWS_COUNT_STAR  arg = the frame: its rows; column must be 0; INT64, never NULL
 *     RJ_WIN_ROWS_COUNT  non-NULL values of an INT32 / INT64 / FP64 column in the frame; INT64, never NULL
 *     RJ_WIN_ROWS_SUM    sum of the non-NULL values of an INT32 / INT64 column in the frame, wrapping
 *                        modulo 2^64; INT64; NULL if the frame has no non-NULL value
 *     RJ_WIN_ROWS_MIN / RJ_WIN_ROWS_MAX  over the non-NULL values of an INT32 / INT64 / FP64 column in the
 *                        frame; the column's type; NULL if the frame has none.  FP64 orders by the sort
 *                        encoding and the result is the canonical value, as for RJ_WIN_MIN / RJ_WIN_MAX.
 *   An empty frame gives COUNT 0 and NULL for SUM / MIN / MAX; NULL is decided by the count of non-NULL
 *   values, never by a sentinel: an INT64_MAX under MIN next to NULLs comes out as a value.  A ROWS_SUM /
 *   ROWS_MIN / ROWS_MAX column is nullable when the child column is, or when the frame can miss the
 *   current row (lo > 0 or hi < 0): the plan decides that, never the data.
 *   RJ_ERR_ARG: a function of this section with a NULL RJ_WINDOW_ARGS; a frame with lo > hi, with lo =
 *   RJ_WIN_UNBOUNDED_FOLLOWING or with hi = RJ_WIN_UNBOUNDED_PRECEDING; LAG / LEAD with k < 0 or arg.hi
 *   != 0; NTILE with n < 1 or arg.hi != 0; NTILE or ROWS_COUNT_STAR with a column other than 0; a column
 *   out of range; a declared type other than the rules above give; a function code that rj_win_func
 *   does not define (9 .. 15, and everything above RJ_WIN_ROWS_MAX).
 *   RJ_ERR_UNSUPPORTED: a VARCHAR column under any function of this section (a row id cannot say
 *   NULL, and its pages are not read here); ROWS_SUM over an FP64 column.
 *   As above the node is checked before its child's rows are looked at.
 *
 * Computed columns (scalar expressions in a select list or under an aggregate; no reference counterpart).
 * RJ_NODE_MAP has ONE child, `left`; `build_left`, `base_table_id` and `left_attr` are ignored.
 *   Program: rj_node cannot grow, so RJ_MAP_N_OPS(node) = `right` and RJ_MAP_OPS(node) = `right_attr` as a
 *   `const rj_expr_op*` that stays valid during the call.  The program is ONE postfix list that holds any
 *   number of expressions: RJ_X_OUT pops the top of the stack and ends expression number e = 0, 1, 2 ...
 *   in order of appearance; after an RJ_X_OUT the stack must be empty.  rj_expr_op::column indexes the
 *   CHILD's outputs.
 *   Outputs (the bit layout of RJ_AGG_OUT): out_idx[k] = RJ_MAP_OUT(RJ_MAP_COL, c) passes child column c
 *   through — a plain column index; the child column's type, bits and nullability; a VARCHAR column passes
 *   through as row ids; nothing is copied.  out_idx[k] = RJ_MAP_OUT(RJ_MAP_EXPR, e) is expression e.  An
 *   expression may be named by several outputs; one that no output names is RJ_ERR_ARG.
 *   Values on the stack are I64 or F64 (typed by the host), each with a NULL flag:
 *     RJ_X_COL (column)      INT32 sign-extends to I64; INT64 -> I64; FP64 -> F64; NULL where the column is
 *     RJ_X_INT (ivalue), RJ_X_F64 (ivalue = the bits), RJ_X_NULL (column = RJ_INT64 or RJ_FP64: a typed
 *                            NULL)  literals
 *     RJ_X_ADD SUB MUL DIV MOD, RJ_X_NEG, RJ_X_ABS  both operands of ONE type (mixed is RJ_ERR_ARG: cast
 *                            first); NULL if an operand is NULL
 *     RJ_X_EQ NEQ LT GT LEQ GEQ  both of one type -> I64 0 / 1; NULL if an operand is NULL; F64 compares
 *                            IEEE-wise, as RJ_NODE_SELECT does
 *     RJ_X_AND, RJ_X_OR, RJ_X_NOT  integer operands, true = non-zero; Kleene's three-valued logic:
 *                            NULL AND 0 = 0, NULL AND 1 = NULL, NULL OR 1 = 1, NULL OR 0 = NULL, NOT NULL = NULL
 *     RJ_X_IS_NULL, RJ_X_IS_NOT_NULL  any type -> 0 / 1, never NULL
 *     RJ_X_COALESCE (a, b)   same type; a unless it is NULL, then b
 *     RJ_X_CASE (c, a, b)    c integer, a and b of the same type; a where c is non-NULL and non-zero, else
 *                            b; all three are always evaluated
 *     RJ_X_TO_I64, RJ_X_TO_F64  casts; to the value's own type the identity
 *     RJ_X_OUT               ends an expression
 *   Integer arithmetic wraps modulo 2^64, as RJ_AGG_SUM does: NEG and ABS of INT64_MIN give INT64_MIN; DIV
 *   truncates toward zero, MOD takes the sign of the dividend; a zero divisor gives NULL, never an error
 *   and never a trap; INT64_MIN / -1 is INT64_MIN and INT64_MIN % -1 is 0.
 *   F64 arithmetic is IEEE-754 binary64, round to nearest even, every op rounded once (no contraction into
 *   FMA, no fast-math, denormals kept); division is correctly rounded and x / 0.0 is +-inf or NaN, not
 *   NULL; NEG flips the sign bit, ABS clears it; MOD on F64 is RJ_ERR_ARG.
 *   Casts: TO_F64 of an I64 rounds to nearest even; TO_I64 of an F64 truncates toward zero and gives NULL
 *   for a NaN and for a value outside [-2^63, 2^63).
 *   An F64 value that is a NaN when RJ_X_OUT pops it comes out as 0x7ff8000000000000 (NaN payloads differ
 *   between hosts and the device).  Nothing else is canonicalised: -0.0 stays -0.0, and a passed-through
 *   column keeps its bits.
 *   Declared result types: an I64 expression INT64, or INT32 (the low 32 bits, wrapping); an F64
 *   expression FP64; anything else is RJ_ERR_ARG.  A computed column is nullable unless the program shows
 *   that it cannot be NULL.
 *   Rows: exactly the child's rows, each once; output row i is computed from row i of the child in the
 *   order the child's rows have on the device.  An empty child gives 0 rows with the declared types and
 *   zero pages.  RJ_MAP_N_OPS == 0 with only pass-through outputs is a projection and launches nothing.
 *   Order: with a SCAN child the result is in the table's row order.  A MAP passes the root's order promise
 *   down: when a MAP is the root, or every ancestor of it up to the root is a MAP, a SORT / GROUP / WINDOW
 *   child delivers its rows in the order it promises at the root and the MAP keeps it (so ORDER BY k LIMIT n
 *   below a MAP computes n rows).  Below any other kind the result is an ordinary relation.
 *   RJ_ERR_ARG: an unknown opcode; a column out of range; operands of different types; a non-integer
 *   operand of AND / OR / NOT or CASE's condition; MOD on F64; RJ_X_NULL with another type code; stack
 *   underflow; a non-empty stack after RJ_X_OUT or at the end of the program; a program that does not end
 *   in RJ_X_OUT; n_ops != 0 with a NULL pointer; an output that names an expression that does not exist;
 *   an expression that no output names; a declared-type mismatch.  RJ_ERR_UNSUPPORTED: RJ_X_COL on a
 *   VARCHAR column; more than RJ_MAP_MAX_OPS ops; a stack deeper than RJ_MAP_MAX_DEPTH; more than
 *   2^32 - 16 child rows.  The node is checked before its child's rows are looked at.
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.  A
 *   library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").
 *
 * Set operations (UNION / INTERSECT / EXCEPT [ALL]; no reference counterpart).
 * RJ_NODE_SETOP has TWO children, `left` and `right`; `build_left`, `base_table_id` and `right_attr` are
 *   ignored.  rj_node cannot grow, so RJ_SETOP_OP(node) = `left_attr` is the operation (rj_setop).
 *   Outputs: out_idx[k] = RJ_SETOP_OUT(l, r) pairs output column k with column l of the LEFT child's
 *   outputs and column r of the RIGHT child's (SQL pairs by position; the plan carries the pairs so that
 *   neither child needs a projection in front of it).  out_type[k] is the declared type, and BOTH columns
 *   must have exactly that type: there is no implicit cast, an RJ_NODE_MAP below does that.  Pairs may
 *   repeat and may come in any order.
 *   Row and equality: a row is the tuple of the n_out output values.  Two rows are equal when they tie in
 *   every column under rj_debug_sort_key's encoding — the grouping equalities of RJ_NODE_GROUP: NULL =
 *   NULL per column, -0.0 = +0.0, NaN = NaN.
 *   Multiplicities: for a row value with l copies on the left and r on the right the result holds
 *     RJ_SET_UNION_ALL      l + r
 *     RJ_SET_UNION          1 if l + r > 0
 *     RJ_SET_INTERSECT      1 if l > 0 and r > 0
 *     RJ_SET_INTERSECT_ALL  min(l, r)
 *     RJ_SET_EXCEPT         1 if l > 0 and r == 0
 *     RJ_SET_EXCEPT_ALL     max(l - r, 0)
 *   copies.
 *   Values: UNION ALL keeps every value's own bits, nothing is canonicalised.  The five other operations
 *   output the run's CANONICAL value as RJ_NODE_GROUP does (rj_debug_sort_key_value): +0.0 for either
 *   zero, 0x7ff8000000000000 for any NaN, NULL for NULL.  Their result is therefore one deterministic
 *   multiset, whatever order the children's rows have and whichever side a copy came from.
 *   Nullability: an output column is nullable when either paired column is (decided by the children's
 *   columns, never by the data).
 *   Order: the five sorting operations give their rows ordered by the output columns, the first most
 *   significant, ascending, NULLs last, as RJ_NODE_SORT orders rows.  UNION ALL gives the left child's
 *   rows followed by the right child's, each in the order that child has on the device: for SCAN
 *   children the table order, otherwise unspecified.  As for RJ_NODE_SORT the order is promised ONLY
 *   when the node is the plan's root; below another node the result is an ordinary relation, and a
 *   parent of any kind may use every column of it, as a key too.  The node never passes an order promise
 *   down to its children.
 *   Empty inputs give the natural result: INTERSECT with an empty side 0 rows, EXCEPT ALL with an empty
 *   right the left rows, canonicalised.  0 result rows come with the declared types and zero pages.
 *   RJ_ERR_ARG: an operation code above RJ_SET_EXCEPT_ALL; n_out == 0; a column out of range on either
 *   side; the two columns of a pair, or the declared type, disagreeing.
 *   RJ_ERR_UNSUPPORTED: more than RJ_SORT_MAX_KEYS DISTINCT pairs in one of the five sorting operations
 *   (UNION ALL takes any number); a VARCHAR pair in a sorting operation (a VARCHAR value travels as a row
 *   id, its pages are not read here); a VARCHAR pair in UNION ALL whose two columns do not come from the
 *   same base-table column (one row-id column cannot point into two tables); more than 2^32 - 16 rows in
 *   the two children together.  A VARCHAR pair of UNION ALL from ONE base-table column is supported
 *   (... FROM t WHERE a UNION ALL ... FROM t WHERE b): the row ids are concatenated.  (A child without rows
 *   that is not a scan holds no row id and pairs with any VARCHAR column.)
 *   The node is checked after its children ran but before their rows are looked at: empty children do
 *   not hide an error.
 *   rj_execute_sharded refuses plans that hold the kind (RJ_ERR_UNSUPPORTED), rj_plan_shardable
 *   reports it, and rj_execute on a multi-device context runs such a plan on its first device.  A
 *   library older than this kind rejects it with RJ_ERR_ARG ("bad node kind").                 */
typedef enum rj_node_kind {
    RJ_NODE_SCAN = 0,
    RJ_NODE_JOIN = 1,
    RJ_NODE_SEMI = 2, /* preserved rows with a partner on the filter side    */
    RJ_NODE_ANTI = 3, /* preserved rows without one                          */
    RJ_NODE_OUTER = 4, /* inner join + unmatched preserved rows, NULL-padded */
    RJ_NODE_FULL = 5,  /* inner join + unmatched rows of BOTH sides, padded  */
    RJ_NODE_AGG = 6,   /* GROUP BY left_attr of the one child `left`         */
    RJ_NODE_SELECT = 7, /* rows of the one child `left` that pass a predicate */
    RJ_NODE_SORT = 8,   /* ORDER BY / LIMIT / OFFSET over the one child `left` */
    RJ_NODE_GROUP = 9,  /* GROUP BY any keys, or none, over the one child `left` */
    RJ_NODE_WINDOW = 10, /* window functions OVER (PARTITION BY / ORDER BY) over the one child `left` */
    RJ_NODE_MAP = 11,    /* computed columns (scalar expressions) over the one child `left` */
    RJ_NODE_SETOP = 12   /* UNION / INTERSECT / EXCEPT [ALL] of the two children `left` and `right` */
} rj_node_kind;

/* Aggregate functions of RJ_NODE_AGG / RJ_NODE_GROUP and the encoding of their out_idx values. */
typedef enum rj_agg_func {
    RJ_AGG_KEY        = 0,
    RJ_AGG_COUNT_STAR = 1,
    RJ_AGG_COUNT      = 2,
    RJ_AGG_SUM        = 3,
    RJ_AGG_MIN        = 4,
    RJ_AGG_MAX        = 5,
    /* (6 and 7 are not assigned) */
    RJ_AGG_FSUM       = 8 /* RJ_NODE_GROUP only: the exactly rounded sum of an FP64 column */
} rj_agg_func;
#define RJ_AGG_OUT(func, col) (((uint64_t)(func) << 56) | (uint64_t)(col))
#define RJ_AGG_FUNC(x) ((uint32_t)((uint64_t)(x) >> 56))
#define RJ_AGG_COL(x) ((uint64_t)(x) & 0x00ffffffffffffffull)

typedef struct rj_node {
    int32_t         kind;          /* rj_node_kind                            */
    int32_t         build_left;    /* JoinNode::build_left (0/1)              */
    uint64_t        base_table_id; /* ScanNode::base_table_id                 */
    uint64_t        left, right;   /* JoinNode child node indices             */
    uint64_t        left_attr, right_attr;
    uint64_t        n_out;
    const uint64_t* out_idx;       /* [n_out] */
    const int32_t*  out_type;      /* [n_out] rj_dtype */
} rj_node;

/* The predicate of an RJ_NODE_SELECT node (`node`: a const rj_node*), carried in integer fields. */
#define RJ_SELECT_N_OPS(node) ((node)->right)
#define RJ_SELECT_OPS(node) ((const rj_filter_op*)(uintptr_t)(node)->right_attr)

/* The keys, limit and offset of an RJ_NODE_SORT node (`node`: a const rj_node*). */
typedef struct rj_sort_key {
    int32_t column; /* index into the child's outputs */
    int32_t flags;  /* RJ_SORT_DESC | RJ_SORT_NULLS_FIRST */
} rj_sort_key;
#define RJ_SORT_DESC 1
#define RJ_SORT_NULLS_FIRST 2
#define RJ_SORT_MAX_KEYS 8
#define RJ_SORT_NO_LIMIT UINT64_MAX
#define RJ_SORT_N_KEYS(node) ((node)->right)
#define RJ_SORT_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)
#define RJ_SORT_LIMIT(node) ((node)->left_attr)
#define RJ_SORT_OFFSET(node) ((node)->base_table_id)

/* The keys of an RJ_NODE_GROUP node (`node`: a const rj_node*): rj_sort_key as above. */
#define RJ_GROUP_N_KEYS(node) ((node)->right)
#define RJ_GROUP_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)

/* The keys of an RJ_NODE_WINDOW node (`node`: a const rj_node*): rj_sort_key as above; the first
 * RJ_WINDOW_N_PART of the RJ_WINDOW_N_KEYS keys are PARTITION BY keys, the rest ORDER BY keys. */
#define RJ_WINDOW_N_KEYS(node) ((node)->right)
#define RJ_WINDOW_KEYS(node) ((const rj_sort_key*)(uintptr_t)(node)->right_attr)
#define RJ_WINDOW_N_PART(node) ((node)->left_attr)

/* Functions of RJ_NODE_WINDOW and the encoding of its out_idx values (the bit layout of RJ_AGG_OUT). */
typedef enum rj_win_func {
    RJ_WIN_COL        = 0, /* a child column passes through */
    RJ_WIN_ROW_NUMBER = 1,
    RJ_WIN_RANK       = 2,
    RJ_WIN_DENSE_RANK = 3,
    RJ_WIN_COUNT_STAR = 4,
    RJ_WIN_COUNT      = 5,
    RJ_WIN_SUM        = 6,
    RJ_WIN_MIN        = 7,
    RJ_WIN_MAX        = 8,
    /* 9 .. 15 are not assigned.  The functions below take an rj_win_arg each (RJ_WINDOW_ARGS). */
    RJ_WIN_LAG = 16, RJ_WIN_LEAD = 17, RJ_WIN_FIRST_VALUE = 18, RJ_WIN_LAST_VALUE = 19, RJ_WIN_NTILE = 20,
    RJ_WIN_ROWS_COUNT_STAR = 21, RJ_WIN_ROWS_COUNT = 22, RJ_WIN_ROWS_SUM = 23, RJ_WIN_ROWS_MIN = 24, RJ_WIN_ROWS_MAX = 25
} rj_win_func;
#define RJ_WIN_OUT(func, col) (((uint64_t)(func) << 56) | (uint64_t)(col))
#define RJ_WIN_FUNC(x) ((uint32_t)((uint64_t)(x) >> 56))
#define RJ_WIN_COL(x) ((uint64_t)(x) & 0x00ffffffffffffffull)

/* The argument of one output of an RJ_NODE_WINDOW node whose function is RJ_WIN_LAG or above: a ROWS
 * frame BETWEEN lo AND hi as signed offsets from the current row (negative = PRECEDING), the offset k
 * of LAG / LEAD in lo, the bucket count of NTILE in lo.  RJ_WINDOW_ARGS(node) points to n_out of
 * them, entry k for output k, and is read only when such a function is present. */
typedef struct rj_win_arg { int64_t lo, hi; } rj_win_arg;
#define RJ_WIN_UNBOUNDED_PRECEDING INT64_MIN
#define RJ_WIN_UNBOUNDED_FOLLOWING INT64_MAX
#define RJ_WINDOW_ARGS(node) ((const rj_win_arg*)(uintptr_t)(node)->base_table_id)

/* The program of an RJ_NODE_MAP node (`node`: a const rj_node*) and the encoding of its out_idx values
 * (the bit layout of RJ_AGG_OUT). */
typedef enum rj_expr_opcode {
    RJ_X_COL = 0, RJ_X_INT = 1, RJ_X_F64 = 2, RJ_X_NULL = 3,
    RJ_X_ADD = 4, RJ_X_SUB = 5, RJ_X_MUL = 6, RJ_X_DIV = 7, RJ_X_MOD = 8, RJ_X_NEG = 9, RJ_X_ABS = 10,
    RJ_X_EQ = 11, RJ_X_NEQ = 12, RJ_X_LT = 13, RJ_X_GT = 14, RJ_X_LEQ = 15, RJ_X_GEQ = 16,
    RJ_X_AND = 17, RJ_X_OR = 18, RJ_X_NOT = 19, RJ_X_IS_NULL = 20, RJ_X_IS_NOT_NULL = 21,
    RJ_X_COALESCE = 22, RJ_X_CASE = 23, RJ_X_TO_I64 = 24, RJ_X_TO_F64 = 25, RJ_X_OUT = 26
} rj_expr_opcode;
typedef struct rj_expr_op {
    int32_t op;     /* rj_expr_opcode */
    int32_t column; /* RJ_X_COL: index into the child's outputs; RJ_X_NULL: RJ_INT64 or RJ_FP64 */
    int64_t ivalue; /* RJ_X_INT: the literal; RJ_X_F64: the bits of the literal */
} rj_expr_op;
#define RJ_MAP_MAX_OPS 128
#define RJ_MAP_MAX_DEPTH 8
#define RJ_MAP_N_OPS(node) ((node)->right)
#define RJ_MAP_OPS(node) ((const rj_expr_op*)(uintptr_t)(node)->right_attr)
typedef enum rj_map_func {
    RJ_MAP_COL  = 0, /* a child column passes through */
    RJ_MAP_EXPR = 1  /* expression number RJ_MAP_ARG(x) of the program */
} rj_map_func;
#define RJ_MAP_OUT(func, x) (((uint64_t)(func) << 56) | (uint64_t)(x))
#define RJ_MAP_FUNC(x) ((uint32_t)((uint64_t)(x) >> 56))
#define RJ_MAP_ARG(x) ((uint64_t)(x) & 0x00ffffffffffffffull)

/* The operation of an RJ_NODE_SETOP node (`node`: a const rj_node*) and the encoding of its out_idx
 * values: the paired columns of the left and of the right child. */
typedef enum rj_setop { RJ_SET_UNION_ALL = 0, RJ_SET_UNION = 1, RJ_SET_INTERSECT = 2,
                        RJ_SET_INTERSECT_ALL = 3, RJ_SET_EXCEPT = 4, RJ_SET_EXCEPT_ALL = 5 } rj_setop;
#define RJ_SETOP_OP(node)        ((node)->left_attr)
#define RJ_SETOP_OUT(lcol, rcol) (((uint64_t)(rcol) << 32) | (uint64_t)(uint32_t)(lcol))
#define RJ_SETOP_LCOL(x)         ((uint32_t)(x))
#define RJ_SETOP_RCOL(x)         ((uint32_t)((uint64_t)(x) >> 32))

/* One Column (include/plan.h:60-100): `pages[i]` points at an 8192-byte Page. */
typedef struct rj_column {
    int32_t            type;    /* rj_dtype */
    uint64_t           n_pages;
    const void* const* pages;   /* [n_pages] host pointers, each RJ_PAGE_SIZE bytes */
} rj_column;

/* One ColumnarTable (include/plan.h:102-105). */
typedef struct rj_input {
    uint64_t         num_rows;
    uint64_t         n_cols;
    const rj_column* cols;
} rj_input;

typedef struct rj_plan {
    uint64_t        n_nodes;
    const rj_node*  nodes;
    uint64_t        n_inputs;
    const rj_input* inputs; /* may be NULL for rj_execute_resident */
    uint64_t        root;
} rj_plan;

/* --------------------------------------------------------------- context --
 * rj_context_create ↔ Contest::build_context() (src/execute.cpp:326-328)
 * rj_context_destroy ↔ Contest::destroy_context() (src/execute.cpp:330)      */
typedef struct rj_context rj_context;

/* Multi-GPU (no reference counterpart: the reference is one CPU process).
 * A context may own several devices of this process (`devices`), and/or be one member of a job
 * that spans several processes (`world_size` > number of local devices, one process per GPU as
 * under torchrun).  Every device is one RANK of the job; a sharded join partitions both inputs
 * by key hash, re-distributes them with ONE all-to-all and joins locally on every rank.
 * The exchange runs over direct peer copies (all ranks in this process) or RCCL (several
 * processes; the communicator is created from `comm_id`, which one process makes with
 * rj_comm_id_create and hands to all others through any channel it likes).               */
#define RJ_COMM_ID_BYTES 128
typedef struct rj_comm_id { char bytes[RJ_COMM_ID_BYTES]; } rj_comm_id;
int rj_comm_id_create(rj_comm_id* out);

enum { RJ_EXCHANGE_AUTO = 0, RJ_EXCHANGE_P2P = 1, RJ_EXCHANGE_RCCL = 2 };

typedef struct rj_config {
    int32_t  device;      /* HIP device ordinal; -1 = current device (ignored when n_devices > 0) */
    int32_t  profile;     /* 1: HIP events around the data-moving kernels,
                             2: around every launch; 0: none                   */
    void*    stream;      /* hipStream_t to launch on; NULL = library-owned (single device only) */
    int32_t  radix_bits;  /* total radix bits; 0 = auto from build cardinality; at most 21 (clamped) */
    int32_t  n_devices;   /* 0 or 1: one device (`device`); N > 1: this context owns devices[0..N) */
    const int32_t* devices;   /* [n_devices] HIP ordinals; an ordinal may repeat (virtual ranks
                                 on one GPU: tests on a single-GPU box)                       */
    int32_t  world_size;  /* ranks of the whole job; 0 = the local devices only               */
    int32_t  rank_base;   /* global rank of the first local device (local device i = rank_base+i) */
    const rj_comm_id* comm_id;  /* required when world_size > local devices                  */
    int32_t  exchange;    /* RJ_EXCHANGE_*                                                     */
    int32_t  flags;       /* RJ_CTX_*                                                          */
} rj_config;

/* rj_config.flags.  RJ_CTX_PREWARM: pay the one-off costs of the first rj_execute inside
 * rj_context_create instead — pinned staging for uploads and result copies, the upload stream,
 * the host worker threads, the code objects of the kernels (HIP loads them at first launch).
 * Contest::build_context() sets it: the harness times build_context once
 * (reference tests/read_sql.cpp:1279-1283) and execute once per query (:1234-1236), so set-up
 * cost belongs there, not into the first query.                                              */
enum { RJ_CTX_PREWARM = 1 };

int         rj_context_create(rj_context** out, const rj_config* cfg /* may be NULL */);
void        rj_context_destroy(rj_context* ctx); /* a handle from rj_context_device() is owned by
                                                     its group context: destroying it is a no-op */
const char* rj_last_error(const rj_context* ctx); /* ctx may be NULL: last create error */
int         rj_abi_version(void);
/* Local devices of a context and the per-device context of each (owned by `ctx`; valid for all
 * single-device entry points: tables are uploaded / adopted and results fetched per device).  */
uint32_t    rj_context_n_devices(const rj_context* ctx);
rj_context* rj_context_device(rj_context* ctx, uint32_t i);

/* ---------------------------------------------------------------- tables --
 * A device-resident ColumnarTable: the Page images of every fixed-width
 * column live contiguously in HBM; VARCHAR pages stay on the host (they are
 * only ever gathered at the root, never joined on).                          */
typedef struct rj_table rj_table;

/* Copy host pages into HBM (pinned staging + async H2D).                     */
int  rj_table_upload(rj_context* ctx, const rj_input* host, rj_table** out);

/* Adopt page images that already sit in HBM: dev_pages[c] is a device pointer
 * to n_pages[c] contiguous 8192-byte pages of column c (NULL for VARCHAR
 * columns, which then must not be referenced).  No copy; caller keeps
 * ownership and must keep the memory alive while the table is in use.        */
int  rj_table_adopt_device(rj_context* ctx, uint64_t num_rows, uint64_t n_cols,
                           const int32_t* col_type, const void* const* dev_pages,
                           const uint64_t* n_pages, rj_table** out);
void rj_table_release(rj_context* ctx, rj_table* t);

/* ---------------------------------------------------------------- ingest --
 * rj_table_from_csv ↔ Table::from_csv(attributes, path, filter) (reference include/table.h:19-22,
 * src/build_table.cpp:135-304) with the CSV text already in host memory and the dialect the
 * harness uses (escape '\\', separator ',', no header, no trailing comma: :231; parser
 * src/csv_parser.cpp:3-175): the text is parsed ON THE DEVICE (quote-aware record / field
 * boundaries, typed fields, empty field = NULL as in TableParser::on_field :31-35), the filter is
 * evaluated on the device, and the rows that pass are packed into Page images in HBM with the
 * page-fill rule of ColumnInserter (reference include/plan.h:151-335) — the resident table a
 * ScanNode then reads without any upload.  Runs BEFORE execute() in the harness and is untimed
 * there (tests/read_sql.cpp:1100-1107,1232-1236): SURVEY.md §8(f)#4.
 * Column types: INT32, INT64, FP64, VARCHAR.  FP64 fields become the double nearest to the decimal
 * text, as std::from_chars does (build_table.cpp:57-64): the device decides all plain numbers
 * (sign, digits, point, exponent) by the Eisel-Lemire algorithm; "inf" / "nan", fields with
 * characters behind the number and the rare text whose rounding 128 bits cannot settle are
 * handed to the host's std::from_chars.  At most 2^32 - 16 bytes of text.
 * Errors (RJ_ERR_DATA) as the reference raises them: "CSV parse error" (a record with another
 * number of fields than n_cols, a quote left open: csv_parser.h:9-14, build_table.cpp:236,243),
 * "parse integer error" (:42-44), "parse float error" (:59-61: not a number, or a value no
 * double represents — overflow, or non-zero text that rounds to zero).  A text with several
 * errors raises the structural one first, then the integer, then the float one (the reference
 * raises whichever comes first in the text).
 *
 * filter: a postfix program over the table's columns (reference include/statement.h,
 * src/statement.cpp:46-135,186-201) — comparison and IS [NOT] NULL leaves push a row bitmap,
 * RJ_F_AND / RJ_F_OR pop two, RJ_F_NOT pops one; n_filter_ops == 0 keeps every row.  NULL
 * semantics are the reference's bitmap arithmetic: a comparison is false on NULL, NOT flips every
 * bit (so NOT (x < 5) holds for NULL x).  Anything else a caller wants to filter by comes in as
 * an RJ_F_HOST_BITMAP leaf, evaluated by the caller: bit r (LSB first) of `bytes` = row r of the
 * CSV passes.                                                                                   */
typedef enum rj_filter_opcode {
    RJ_F_EQ = 0, RJ_F_NEQ = 1, RJ_F_LT = 2, RJ_F_GT = 3, RJ_F_LEQ = 4, RJ_F_GEQ = 5, /* column <op> literal.  INT32 / INT64
                                        columns: ivalue (an INT32 column compares with (int32_t)ivalue: statement.cpp:55);
                                        FP64 columns: ivalue holds the BITS of the double literal, compared as doubles
                                        are (statement.cpp:91-107: a NaN equals nothing);
                                        VARCHAR columns: the ivalue bytes at `bytes`, compared as std::string does
                                        (unsigned bytes, then length: statement.cpp:117-126)                    */
    RJ_F_IS_NULL = 6, RJ_F_IS_NOT_NULL = 7,                   /* any column                                   */
    RJ_F_HOST_BITMAP = 8,
    RJ_F_AND = 9, RJ_F_OR = 10, RJ_F_NOT = 11,
    RJ_F_LIKE = 12, RJ_F_NOT_LIKE = 13, /* VARCHAR column LIKE / NOT LIKE the ivalue bytes at `bytes` ('%' any run,
                                           '_' any one character) — what the reference asks RE2 for
                                           (statement.h:118-161: '%' -> ".*", '_' -> ".", full match, UTF-8, '.'
                                           never matches a newline); false on NULL, both of them
                                           (inner_column.h:518-562); at most 63 pattern characters         */
    RJ_F_COL_EQ = 14, RJ_F_COL_NEQ = 15, RJ_F_COL_LT = 16, RJ_F_COL_GT = 17, RJ_F_COL_LEQ = 18, RJ_F_COL_GEQ = 19
                                        /* RJ_NODE_SELECT only (rj_table_from_csv: "bad filter opcode"): column <op>
                                           column.  `column` is the left operand, `ivalue` the right operand's column
                                           index; both INT32, both INT64 or both FP64; false if either side is NULL;
                                           FP64 compares IEEE-wise                                                  */
} rj_filter_opcode;

typedef struct rj_filter_op {
    int32_t        op;          /* rj_filter_opcode */
    int32_t        column;      /* leaves */
    int64_t        ivalue;      /* comparison leaves: the literal, or the length of a string literal;
                                   RJ_F_COL_*: the right operand's column index                      */
    const uint8_t* bytes;       /* RJ_F_HOST_BITMAP: (rows + 7) / 8 bytes, rows = records of the CSV;
                                   string comparison: the literal's bytes                            */
} rj_filter_op;

int rj_table_from_csv(rj_context* ctx, const char* text, uint64_t n_bytes, uint64_t n_cols,
                      const int32_t* col_type, const rj_filter_op* filter, uint64_t n_filter_ops,
                      rj_table** out);
/* A resident table's shape and pages (tests compare them with the reference's fill rule). */
/* The FP64 field parser of rj_table_from_csv on ONE field, run on the host (no device needed;
 * tests): 0 = *bits holds the double, 1 = out of range ("parse float error"), 2 = left to
 * std::from_chars.                                                                             */
int rj_debug_parse_fp64(const char* field, uint64_t n, uint64_t* bits);

/* The order-preserving key encoding of RJ_NODE_SORT, run on the host (the kernels share the code):
 * for a value of `type` (RJ_INT32 / RJ_INT64 / RJ_FP64; `bits` = its bits, an INT32's in the low
 * word) under `flags` (RJ_SORT_DESC | RJ_SORT_NULLS_FIRST), row a sorts before row b exactly when
 * (null_digit, key) of a is below that of b as a pair of unsigned numbers, and they tie when the
 * pairs are equal.  INT32: bits ^ 2^31 (a 32-bit key); INT64: bits ^ 2^63; FP64: -0.0 becomes +0.0
 * and every NaN one NaN above +inf, then bits ^ (sign ? ~0 : 2^63); RJ_SORT_DESC: the bitwise NOT of
 * those bits.  null_digit: the NULL flag oriented by RJ_SORT_NULLS_FIRST; a NULL's key is 0.
 * Needs neither a context nor a GPU.  RJ_ERR_ARG: another type, other flag bits, a NULL pointer.  */
int rj_debug_sort_key(int32_t type, int32_t flags, uint64_t bits, int is_null, uint64_t* key, uint32_t* null_digit);
/* Its inverse for a non-NULL key, run on the host (the kernels of RJ_NODE_GROUP share the code): *bits =
 * the CANONICAL value bits of the values whose key under `flags` is `key` — an INT32's in the low
 * word; +0.0 for the key of the zeros, 0x7ff8000000000000 for the key of the NaNs.  Needs neither a
 * context nor a GPU (an INT32 key is its low 32 bits).  RJ_ERR_ARG: another type, other flag bits, a
 * NULL pointer.                                                                                     */
int rj_debug_sort_key_value(int32_t type, int32_t flags, uint64_t key, uint64_t* bits);
/* The frame arithmetic of RJ_NODE_WINDOW's ROWS frames, run on the host (the k_frame_* kernels share the
 * code): the row at position i of a partition [ps, pe] (all three below 2^32) under ROWS BETWEEN lo
 * AND hi as signed offsets.  -> 1 and the frame [*a, *b] = [max(ps, i + lo), min(pe, i + hi)], or 0
 * when that is empty (a and b are then untouched) or a pointer is NULL.  Needs neither a context nor
 * a GPU.                                                                                             */
int rj_debug_win_frame(uint64_t i, uint64_t ps, uint64_t pe, int64_t lo, int64_t hi, uint64_t* a, uint64_t* b);
/* RJ_WIN_NTILE on the host (the kernel shares the code): the bucket, 1-based, of the row that has r
 * rows of its partition in front of it, the partition having N rows, under NTILE(n).  -> 0 for n < 1
 * or r >= N.  Needs neither a context nor a GPU.                                                      */
int64_t rj_debug_win_ntile(uint64_t r, uint64_t N, int64_t n);
/* RJ_AGG_FSUM of ONE group, run on the host through the add, merge and round functions the kernels
 * call, in blocks of a few thousand values merged as the kernels merge their partial sums: bits[i] =
 * the bits of value i, is_null[i] != 0 = NULL (is_null may be NULL: no NULLs).  *out_bits = the exactly
 * rounded sum's bits, *out_is_null = 1 (and *out_bits = 0) when no value is left, as for n = 0.  Needs
 * neither a context nor a GPU.  RJ_ERR_ARG: a NULL output pointer, or n != 0 without bits.          */
int rj_debug_fsum(const uint64_t* bits, const uint8_t* is_null /* may be NULL */, uint64_t n,
                  uint64_t* out_bits, int32_t* out_is_null);
/* The program of an RJ_NODE_MAP node on ONE row, run on the host: it is validated by the code the
 * executor uses and evaluated through the op functions the kernel calls.  The row has n_cols columns:
 * col_type[c] (rj_dtype), col_bits[c] (the value's bits, an INT32's in the low word), col_null[c] != 0 =
 * NULL.  Expression e (at most out_cap of them are written, *n_out = how many the program holds) leaves
 * out_bits[e], out_null[e] and out_kind[e] = RJ_INT64 for an I64 result, RJ_FP64 for an F64 one (the
 * bits of a NULL result are 0).  Needs neither a context nor a GPU.  Returns the executor's status codes
 * for the program (the outputs of a node are not part of it), the message in rj_last_error(NULL).      */
int rj_debug_map_eval(const rj_expr_op* ops, uint64_t n_ops, uint64_t n_cols, const int32_t* col_type,
                      const uint64_t* col_bits, const uint8_t* col_null, uint64_t out_cap, uint64_t* out_bits,
                      uint8_t* out_null, int32_t* out_kind, uint64_t* n_out);
/* The pass plan of ONE radix partition call, as the library's driver would take it (csrc/rj_radix_plan.cpp): every
 * decision that is taken before the first launch, from the facts of the request, the RJ_TUNE_* variables (read from
 * the environment by this call, as a context reads them when it is made) and a compute-unit count.  Needs neither
 * a context nor a GPU.  RJ_ERR_ARG: a NULL pointer, key_words outside 1..2 or carry_words outside 0..3 or more than
 * 4 words together, more than 32 bits, a single pass of more than 9 bits, a packed word source that is not one
 * key word + one carry word.                                                                                     */
typedef struct rj_partition_request {
    uint64_t n;                        /* rows of the source                                                    */
    int32_t  key_words, carry_words;
    uint32_t bits, shift0;
    int32_t  single_pass;
    int32_t  word_source;              /* 0 = columns, 1 = tuples in word arrays, 2 = ... in packed pairs       */
    int32_t  external;                 /* caller-owned output arrays                                            */
    int32_t  composite;                /* composite digit (stage A of a sharded join)                           */
    uint32_t preseg_nseg, preseg_n_oseg; /* pre-segmented input (stage B): input runs, output segments; 0 = not */
    int32_t  after_offsets;            /* the caller takes the first pass' offsets ahead of its scatter         */
    int32_t  flag_word;                /* a flag word was given: the first pass may be speculative              */
    int32_t  spec2_ok;                 /* ... and the last pass too                                             */
} rj_partition_request;
enum { RJ_PLAN_MAX_PASSES = 4 };
typedef enum rj_plan_mid {             /* how tuples travel between the passes                                  */
    RJ_MID_DENSE = 0, RJ_MID_PACKED = 1, RJ_MID_PACKED_SIDE = 2, RJ_MID_BLOCKED = 3, RJ_MID_AOS3 = 4, RJ_MID_AOS3_SIDE = 5
} rj_plan_mid;
typedef enum rj_plan_last { RJ_LAST_DENSE = 0, RJ_LAST_PACKED = 1, RJ_LAST_AOS3 = 2 } rj_plan_last;
typedef enum rj_plan_offsets {         /* where a pass gets its partition offsets from                          */
    RJ_OFF_FINE = 0, RJ_OFF_HIST = 1, RJ_OFF_SAMPLE = 2, RJ_OFF_CHUNKED = 3
} rj_plan_offsets;
typedef enum rj_plan_hist {            /* the launcher that counts for a pass                                   */
    RJ_HIST_NONE = 0, RJ_HIST_FINE_SRC, RJ_HIST_FINE_WORDS, RJ_HIST_SRC, RJ_HIST_DIGITS, RJ_HIST_AOS3, RJ_HIST_BLOCKED,
    RJ_HIST_PACKED, RJ_HIST_DENSE, RJ_HIST_SAMPLE_SRC, RJ_HIST_LAST_SAMPLE
} rj_plan_hist;
typedef enum rj_plan_scatter {         /* the launcher that writes a pass                                       */
    RJ_SCATTER_SRC = 0, RJ_SCATTER_SRC_PACKED, RJ_SCATTER_DENSE, RJ_SCATTER_PACKED, RJ_SCATTER_BLOCKED, RJ_SCATTER_AOS3,
    RJ_SCATTER_LAST_BLOCKED, RJ_SCATTER_LAST_DENSE
} rj_plan_scatter;
typedef struct rj_partition_pass {
    uint32_t bits, tiles_per_group, xcd_log2, xcd_remap;
    uint32_t nseg_in, n_oseg, n_groups;
    int32_t  offsets, hist, scatter;   /* rj_plan_offsets, rj_plan_hist, rj_plan_scatter                        */
    uint64_t bins;
} rj_partition_pass;
typedef struct rj_partition_plan {
    uint32_t passes;
    uint32_t pbits[RJ_PLAN_MAX_PASSES];
    int32_t  fine, fine_xcd;
    uint32_t fine_grid;
    int32_t  mid, last;                /* rj_plan_mid, rj_plan_last                                             */
    int32_t  spec, spec2;
    uint64_t spec_cap_max, spec2_cap_max;  /* the bounds, whether or not the pass is speculative                */
    uint64_t n_first_out, n_last_out;  /* tuples the first / last pass' output arrays hold                      */
    uint32_t tpg_first, reserved;
    rj_partition_pass pass[RJ_PLAN_MAX_PASSES];
} rj_partition_plan;
int rj_debug_partition_plan(const rj_partition_request* req, uint32_t compute_units, rj_partition_plan* out);
uint64_t rj_table_num_rows(const rj_table* t);
uint64_t rj_table_col_pages(const rj_table* t, uint64_t col);
int      rj_table_copy_pages(rj_context* ctx, const rj_table* t, uint64_t col, void* const* dst, uint64_t n_dst);

/* --------------------------------------------------------------- execute --
 * rj_execute ↔ Contest::execute(const Plan&, void*) (src/execute.cpp:316-324):
 *   inputs are the host pages in plan->inputs; the result pages are produced
 *   on the device and fetched with rj_result_copy_pages.
 * rj_execute_resident: same plan semantics, inputs already in HBM
 *   (plan->inputs ignored; tables[i] ↔ plan.inputs[i]).  With
 *   RJ_EXEC_KEEP_ON_DEVICE the fixed-width result pages stay in HBM.
 * A plan whose root is a scan: the pages of every result column add up to the table's
 *   num_rows rows, whatever the input's pages add up to (rows the input's pages do not
 *   cover are NULL, NULL rows they carry past num_rows are dropped).  A fixed-width
 *   column of full pages without NULLs, and a VARCHAR column whose pages hold exactly
 *   num_rows rows, come back as the input's own page images; any other column is
 *   decoded and encoded again.  The root scan of a table without rows has no pages.  */
typedef struct rj_result rj_result;

enum { RJ_EXEC_KEEP_ON_DEVICE = 1 };

int rj_execute(rj_context* ctx, const rj_plan* plan, rj_result** out);
int rj_execute_resident(rj_context* ctx, const rj_plan* plan, rj_table* const* tables,
                        uint64_t n_tables, int32_t flags, rj_result** out);

uint64_t rj_result_num_rows(const rj_result* r);
uint64_t rj_result_num_cols(const rj_result* r);
int32_t  rj_result_col_type(const rj_result* r, uint64_t col);
uint64_t rj_result_col_pages(const rj_result* r, uint64_t col);
/* Copy column `col` into caller-allocated pages (dst[i] = 8192-byte block,
 * e.g. `new Page` so that Column::~Column, plan.h:95-99, can delete them).   */
int      rj_result_copy_pages(rj_result* r, uint64_t col, void* const* dst, uint64_t n_dst);
/* Device pointer to the contiguous page images of a column whose pages sit in HBM (valid until
 * rj_result_free): fixed-width columns, and VARCHAR columns of large results, which are encoded
 * on the device.  NULL for host-encoded VARCHAR columns and for a result gathered from several
 * devices (rj_execute on a multi-device context: its pages are not one run — use
 * rj_result_copy_pages).                                                     */
const void* rj_result_device_pages(const rj_result* r, uint64_t col);
void     rj_result_free(rj_result* r);

/* ------------------------------------------------------- sharded (multi-GPU)
 * rj_execute on a context that owns several devices shards every JoinNode it can across them
 * (inputs are split by row ranges on the way up, the result is the concatenation of the ranks'
 * pages) and falls back to the first device for plans it cannot shard — the drop-in boundary
 * stays Contest::execute.
 *
 * rj_execute_sharded is the resident form (bench.py, one process per GPU or one process with
 * several): tables[d * n_inputs + i] is the shard of plan input i that lives on local device d
 * (made with rj_table_upload / rj_table_adopt_device on rj_context_device(ctx, d)); the union of
 * all ranks' shards is the input.  out[d] receives local device d's slice of the result (rows
 * whose key hashes to that rank).  Collective: every process of the job must call it with the
 * same plan.  Shardable plans: every JoinNode carries at most one fixed-width non-key column per
 * side (the BASELINE shape), and no node is a semi, anti, outer or full outer join, an
 * aggregation, a selection, a sort, a grouping, a window, a map or a set operation node; others return
 * RJ_ERR_UNSUPPORTED.                                                                          */
int rj_execute_sharded(rj_context* ctx, const rj_plan* plan, rj_table* const* tables,
                       uint64_t n_inputs, int32_t flags, rj_result** out /* [n local devices] */);
/* 1 if rj_execute_sharded (and rj_execute on a multi-device context) can shard this plan, else 0
 * with the reason in `why` (optional, NUL-terminated, at most why_cap bytes).  Looks at the plan
 * only: needs neither a context nor a GPU.  A plan that holds a semi, anti, outer or full outer
 * join, an aggregation, a selection, a sort, a grouping, a window, a map or a set operation node is not
 * shardable; the reason names the kind (RJ_NODE_SEMI / RJ_NODE_ANTI / RJ_NODE_OUTER / RJ_NODE_FULL /
 * RJ_NODE_AGG / RJ_NODE_SELECT / RJ_NODE_SORT / RJ_NODE_GROUP / RJ_NODE_WINDOW / RJ_NODE_MAP /
 * RJ_NODE_SETOP).                                                                              */
int rj_plan_shardable(const rj_plan* plan, char* why, size_t why_cap);

/* The layout of the exchange step, as a pure function of the all-gathered count tensor (host
 * arithmetic only: needs neither a context nor a GPU; this is what the library itself runs between
 * the count all-gather and the all-to-all, exposed so that it can be checked — and rehearsed over
 * any transport, e.g. gloo on CPUs — without one).  Stage A of a sharded join partitions a rank's
 * tuples by (owner rank, first local radix digit) and lays them out owner-major;
 *   counts[(src * world + dst) * subs + sub] = tuples rank `src` holds for owner `dst`, digit `sub`.
 * For rank `rank` (all outputs optional, in TUPLES): send_off/send_cnt[world] = the slice of its
 * stage-A output that goes to each rank; recv_off/recv_cnt[world] = where each source's slice
 * lands in its receive buffer; seg_begin/seg_end[subs * world] = the runs that arrive, listed
 * digit-major (run of digit k from source s at index k * world + s) — the input segments of the
 * next radix pass, `world` of them feeding first-level partition k; part_off[subs + 1] = prefix of
 * those partitions' sizes; n_recv = tuples received.  RJ_ERR_UNSUPPORTED when ANY rank of the
 * world would receive more than 2^32 - 16 tuples (every rank takes that decision alike, before a
 * collective moves data); message in rj_last_error(NULL).                                       */
int rj_exchange_plan(uint32_t world, uint32_t subs, uint32_t rank, const uint64_t* counts,
                     uint64_t* send_off, uint64_t* send_cnt, uint64_t* recv_off, uint64_t* recv_cnt,
                     uint32_t* seg_begin, uint32_t* seg_end, uint32_t* part_off, uint64_t* n_recv);

/* Lower-level pieces of the same path, for callers that run the exchange themselves (e.g.
 * torch.distributed in pyrj.dist, gloo on CPU in the tests).  Tuples are SoA: `key` (int32)
 * plus `carry` (one 32-bit word per tuple, the payload or a row id).                         */
typedef struct rj_tuples {
    uint64_t n;
    void*    key;    /* device, n * 4 bytes  */
    void*    carry;  /* device, n * 4 bytes  */
    uint32_t hashed; /* !=0: `key` holds the library's bijective hash image of the
                        keys (what stage A emits; stage B un-hashes on output)  */
    uint32_t reserved;
} rj_tuples;

/* Stage A: decode (key_col, carry_col) of a resident table and partition the
 * non-NULL-key tuples by destination rank.  The caller provides out->key and
 * out->carry (device buffers with room for the table's num_rows tuples, e.g.
 * torch tensors that then go straight into the all-to-all).  On return they
 * hold the tuples grouped by rank (rank 0 first), out->n the tuple count,
 * out->hashed = 1 and counts[r] the tuples destined for rank r.              */
int  rj_shard_partition(rj_context* ctx, const rj_table* t, uint64_t key_col,
                        uint64_t carry_col, uint32_t n_ranks, rj_tuples* out,
                        uint64_t* counts /* [n_ranks] */);

/* Stage B: inner equi-join of two tuple sets resident in HBM (caller-owned
 * device pointers).  Output columns: key, build carry, probe carry — i.e. the
 * plan Join(build_left=true, out={0,1,3}) over Scan{key,payload} children.
 * skip_rank_bits = log2(n_ranks) top hash bits already consumed by stage A (they are constant
 * on this rank: the radix plan stays below them).                                           */
int  rj_join_tuples(rj_context* ctx, const rj_tuples* build, const rj_tuples* probe,
                    uint32_t skip_rank_bits, int32_t flags, rj_result** out);

/* -------------------------------------------------------------- profiling --
 * With rj_config.profile != 0 every kernel launch is bracketed by HIP events
 * on the launch stream.  rj_profile_read drains them (synchronises).         */
typedef struct rj_kernel_stat {
    char     name[48];
    uint64_t launches;
    double   total_ms;
} rj_kernel_stat;

int  rj_profile_read(rj_context* ctx, rj_kernel_stat* out, uint64_t cap, uint64_t* n);
void rj_profile_reset(rj_context* ctx);

/* Launch log (tests): which kernel template instantiations ran.  on != 0 starts
 * counting every launch of the join kernels per kernel handle, 0 stops; both clear
 * the log.  Off by default (then a launch costs one untaken branch).  A group
 * context logs the launches of all its devices.                                  */
int  rj_debug_launch_log(rj_context* ctx, int on);
/* Newline-separated "<mangled symbol of the kernel handle> <launches>" lines (a
 * handle without a dynamic symbol: "+0x<offset from the library's base>"), NUL-
 * terminated and truncated to cap bytes; *need = bytes the whole text takes.     */
int  rj_debug_launch_read(rj_context* ctx, char* buf, uint64_t cap, uint64_t* need);
/* Block cache (tests): out[0] = bytes in use, out[1] = bytes cached, out[2] = fills done
 * and out[3] = bytes filled under RJ_DEBUG_POISON (both 0 when the knob is off).  A
 * group context reports the sum over its devices.                                   */
int  rj_debug_pool(rj_context* ctx, uint64_t out[4]);

/* Device properties the host side reports next to its numbers. */
typedef struct rj_device_info {
    char     name[128];
    char     arch[64];
    int32_t  compute_units;
    int32_t  wavefront;
    uint64_t hbm_bytes;
    uint64_t lds_per_cu;
    int32_t  device_count;  /* HIP devices visible to this process */
    int32_t  reserved;
} rj_device_info;
int rj_device_query(rj_context* ctx, rj_device_info* out);

#ifdef __cplusplus
}
#endif
#endif /* RJ_H_ */
