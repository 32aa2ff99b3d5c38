"""Python mirror of the graphlily::module operator API on top of the HIP C ABI.

Same class names, method names, argument meaning and blocking behaviour as the reference's
header-only modules, so parity tests read like the reference's tests/test_module_*.cpp:

  BaseModule                  module/base_module.h:10-133
  SpMVModule                  module/spmv_module.h:37-532
  SpMSpVModule                module/spmspv_module.h:27-520
  eWiseAddModule              module/add_scalar_vector_dense_module.h:19-204
  AssignVectorDenseModule     module/assign_vector_dense_module.h:19-246
  AssignVectorSparseModule    module/assign_vector_sparse_module.h:19-335

The C++ twin (the actual drop-in for C++ callers) lives in include/graphlily/module/*.h and calls
the same entry points.  Device buffers are capi.DeviceBuffer handles and play the role of the
public cl::Buffer members (`vector_buf`, `mask_buf`, ...), including being shareable via bind_*.
`compute_reference_results` is deliberately absent: the CPU reference is test infrastructure
(oracle/) and the product never routes through it.
"""
import collections
import os
import sys

import numpy as np

from . import capi
from .capi import IDX_VAL

# ---------------------------------------------------------------- graphlily/global.h
kMulAdd, kLogicalAndOr, kAddMin = 0, 1, 2                    # :83-87
kNoMask, kMaskWriteToZero, kMaskWriteToOne = 0, 1, 2         # :103-107
SemiringType = collections.namedtuple("SemiringType", ["op", "one", "zero"])  # :90-94
UFIXED_INF = 255.0                                           # :79
FLOAT_INF = 999999999.0                                      # :80
ArithmeticSemiring = SemiringType(kMulAdd, 1.0, 0.0)         # :96
LogicalSemiring = SemiringType(kLogicalAndOr, 1.0, 0.0)      # :97
# :99-100 -- the reference ships the ap_ufixed line (zero = 255); with val_t = float the FLOAT_INF
# line is the one to enable.  `zero` is a runtime field here, so either works.
TropicalSemiring = SemiringType(kAddMin, 0.0, FLOAT_INF)
TropicalSemiringUfixed = SemiringType(kAddMin, 0.0, UFIXED_INF)
pack_size = 8                                                # :57
num_hbm_channels = 16                                        # :59
idx_marker = 0xFFFFFFFF                                      # :66


def _fatal(msg):
    """The reference reports errors by printing and exit(EXIT_FAILURE) (xcl2.hpp:40-46)."""
    print(msg, file=sys.stderr)
    raise SystemExit(1)


def make_sparse_vec(indices, vals, head_val=0.0):
    """aligned_sparse_vec_t with the count in [0].index (module/spmspv_module.h:53-60)."""
    indices = np.asarray(indices)
    v = np.zeros(len(indices) + 1, dtype=IDX_VAL)
    v["index"][0] = len(indices)
    v["val"][0] = head_val
    v["index"][1:] = indices
    v["val"][1:] = vals
    return v


def convert_sparse_vec_to_dense_vec(sparse_vector, rng, zero):
    """graphlily/global.h:153-164"""
    dense = np.full(rng, zero, dtype=np.float32)
    nnz = int(sparse_vector["index"][0])
    dense[sparse_vector["index"][1:nnz + 1]] = sparse_vector["val"][1:nnz + 1]
    return dense


class BaseModule:
    # Counts the module calls that write device memory (any module's run / send_* / copy).  An SpMSpVModule remembers the
    # value right after it uploaded a tiny vector; while nothing else has written since, its runs tell the library that
    # the vector is still that tiny one (gl_spmspv_plan_hint_work: one launch instead of two).
    device_writes_ = 0

    def __init__(self, kernel_name="overlay"):
        self.kernel_name_ = kernel_name
        self.target_ = "hw"
        self.device_ = 0
        self.blocking = True  # every reference call ends in command_queue_.finish()

    def get_kernel_name(self):
        return self.kernel_name_

    def set_target(self, target):
        assert target in ("sw_emu", "hw_emu", "hw")  # base_module.h:74-77
        self.target_ = target

    def set_device(self, device):
        self.device_ = int(device)

    def set_up_runtime(self, xclbin_file_path=None):
        """No bitstream on a GPU: the path is accepted and ignored; this selects the device."""
        capi.init(self.device_)

    def copy_buffer_device_to_device(self, src, dst, nbytes):
        BaseModule._wrote(dst)
        capi.copy_d2d(dst, src, nbytes)
        capi.sync()

    @staticmethod
    def _wrote(*buffers):
        """One more module call has written device memory; `buffers` are the ones it wrote (each remembers the call's number:
        SpMSpVModule.get_results_nnz trusts the operator's completion record only while its run is the last writer of
        results_buf)."""
        BaseModule.device_writes_ += 1
        for b in buffers:
            if b is not None:
                b.last_write_ = BaseModule.device_writes_

    def _finish(self, *written):
        BaseModule._wrote(*written)       # every run / send_* of every module ends here
        if self.blocking:
            capi.sync()


class SpMVModule(BaseModule):
    def __init__(self, num_channels=num_hbm_channels, out_buf_len=0, vec_buf_len=0):
        super().__init__()
        # FPGA buffer geometry; kept for signature parity, the GPU tiling is chosen by the plan
        self.num_channels_, self.out_buf_len_, self.vec_buf_len_ = num_channels, out_buf_len, vec_buf_len
        self.mask_type_ = kNoMask
        self.semiring_ = ArithmeticSemiring
        self.csr_matrix_ = None
        self.plan_ = None
        self.row_begin_, self.row_end_ = 0, None
        self.vector_buf = self.mask_buf = self.results_buf = None
        self.plan_flags_ = 0

    def set_semiring(self, semiring):
        self.semiring_ = semiring

    def set_mask_type(self, mask_type):
        self.mask_type_ = mask_type

    def set_row_shard(self, row_begin, row_end):
        """Multi-GPU extension: this device owns rows [row_begin, row_end) of the matrix."""
        self.row_begin_, self.row_end_ = int(row_begin), int(row_end)

    def set_plan_flags(self, flags):
        """Extension: GL_PLAN_* flags for the plans this module creates (before send_matrix_host_to_device), e.g.
        capi.GL_PLAN_REFERENCE_ORDER -- the diagnostic layout that evaluates compute_reference_results' own loop
        (module/spmv_module.h:478-510) on the device -- or capi.GL_PLAN_KEEP_VALUES."""
        self.plan_flags_ = int(flags)

    def get_num_rows(self):
        return self.csr_matrix_.num_rows

    def get_num_cols(self):
        return self.csr_matrix_.num_cols

    def get_nnz(self):
        return int(self.csr_matrix_.adj_indptr[self.csr_matrix_.num_rows])

    def load_and_format_matrix(self, csr_matrix_float, skip_empty_rows=True):
        # skip_empty_rows only changes the FPGA stream encoding; results are identical either way
        self.csr_matrix_ = csr_matrix_float
        self.skip_empty_rows_ = skip_empty_rows

    @staticmethod
    def _plan_flags(op):
        if op == kLogicalAndOr:     # pattern-only entries, x as bits (gl_spmv_bool.hip)
            return capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD
        return capi.GL_PLAN_NO_MULADD if op != kMulAdd else 0

    def _plan_serves(self, op):
        f = self.plan_.flags
        if f & capi.GL_PLAN_REFERENCE_ORDER:
            return True
        if (f & capi.GL_PLAN_BOOLEAN) and op != kLogicalAndOr:
            return False
        return not ((f & capi.GL_PLAN_NO_MULADD) and op == kMulAdd)

    def _make_plan(self):
        m = self.csr_matrix_
        re = m.num_rows if self.row_end_ is None else self.row_end_
        # the semiring known at upload time sizes the LDS split (accumulators vs hot-column table); a later
        # switch to (+,x) on a plan built for the 4-byte semirings re-formats the matrix (see run())
        flags = self._plan_flags(self.semiring_.op) | self.plan_flags_
        if os.environ.get("GRAPHLILY_SPMV_ORDER") == "reference":   # the C++ module layer's switch (spmv_module.h), mirrored
            flags |= capi.GL_PLAN_REFERENCE_ORDER
            self.plan_flags_ |= capi.GL_PLAN_REFERENCE_ORDER
        if flags & capi.GL_PLAN_REFERENCE_ORDER:
            flags = capi.GL_PLAN_REFERENCE_ORDER
        for client in getattr(self, "pull_clients_", ()):   # the old plan is about to go away
            client._attach(None)
        self.plan_ = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data,
                                   self.row_begin_, re, flags)
        for client in getattr(self, "pull_clients_", ()):
            client._attach(self)

    def send_matrix_host_to_device(self):
        m = self.csr_matrix_
        self._make_plan()
        self.results_buf = capi.DeviceBuffer(4 * m.num_rows)
        capi.fill_f32(self.results_buf, 0.0, m.num_rows)  # spmv_module.h:368-369

    @staticmethod
    def _upload_dense(host, n):
        """Fresh n-float buffer holding `host`, zero-padded when it is shorter (device blocks are recycled:
        nothing may be assumed about what a new buffer holds)."""
        host = np.ascontiguousarray(host, dtype=np.float32)[:n]
        buf = capi.DeviceBuffer(4 * n)
        buf.write(host)
        if host.shape[0] < n:
            tail = capi.DeviceBuffer(4 * (n - host.shape[0]), ptr=buf.ptr + 4 * host.shape[0], keepalive=buf)
            capi.fill_f32(tail, 0.0, n - host.shape[0])
        return buf

    def send_vector_host_to_device(self, vector):
        self.vector_buf = self._upload_dense(vector, self.get_num_cols())

    def send_mask_host_to_device(self, mask):
        self.mask_buf = self._upload_dense(mask, self.get_num_rows())

    def bind_mask_buf(self, src_buf):
        self.mask_buf = src_buf

    def bind_vector_buf(self, src_buf):
        self.vector_buf = src_buf

    def bind_results_buf(self, src_buf):
        self.results_buf = src_buf

    def run(self):
        mask = self.mask_buf if self.mask_type_ != kNoMask else None
        if not self._plan_serves(self.semiring_.op):   # semiring switched after upload: re-format
            capi.sync()
            self._make_plan()
        self.plan_.run(self.vector_buf, mask, self.results_buf, self.semiring_.op, self.semiring_.zero,
                       self.mask_type_)
        self._finish(self.results_buf)

    def chain(self, on):
        """Extension (gl_spmv_plan_chain): the caller feeds every result straight back as the next vector and touches neither in
        between (PageRank.pull, SSSP.pull) -- the run's epilogue then prepares the next run's packed x.  -> active?"""
        if self.plan_ is None or not hasattr(self.plan_, "chain"):
            return False
        if on and os.environ.get("GRAPHLILY_SPMV_CHAIN", "1") == "0":      # (A/B and tests: every run launches its helper)
            return False
        return self.plan_.chain(on)

    # extensions for row-sharded (||,&&) runs: x as a bit vector (gl_spmv_plan_bits_words / gl_spmv_run_bits)
    def bits_words(self):
        if self.plan_ is None or (self.plan_.flags & capi.GL_PLAN_REFERENCE_ORDER):
            return 0
        return self.plan_.bits_words() if self._plan_serves(self.semiring_.op) else 0

    def bfs_pull_step(self, bits_in, bits_out, distance_buf, level):
        """Extension (gl_bfs_pull_step): this module's masked (||,&&) run + eWiseAdd(+0) + dense assign(level) of a
        BFS pull iteration in one launch, frontier in and out as bit vectors.  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) for split plans."""
        self.plan_.bfs_pull_step(bits_in, bits_out, distance_buf, level)
        self._finish(bits_out, distance_buf)

    def bfs_parents(self, distance_buf, parent_buf, orphans_buf=None):
        """Extension (gl_bfs_parents): the BFS predecessor tree of the level vector in `distance_buf` (get_num_cols() floats)
        for this module's rows, into `parent_buf` (uint32 words; 0xffffffff = none).  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does)."""
        if self.plan_ is None:
            _fatal("SpMVModule.bfs_parents: send_matrix_host_to_device first")
        self.plan_.bfs_parents(distance_buf, parent_buf, orphans_buf)
        self._finish(parent_buf)

    def cc_labels(self, labels_buf, count_buf=None):
        """Extension (gl_cc_labels): the weakly connected components of this module's rows over get_num_cols() vertices, into
        `labels_buf` (uint32 words: the smallest vertex of each vertex's component); `count_buf`: an optional device word for
        the number of components.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the
        (||,&&) layout does)."""
        if self.plan_ is None:
            _fatal("SpMVModule.cc_labels: send_matrix_host_to_device first")
        self.plan_.cc_labels(labels_buf, count_buf)
        self._finish(labels_buf, count_buf)

    def tc_count(self, total_buf, per_vertex_buf=None):
        """Extension (gl_tc_count): the triangle count of this module's matrix -- rows as strictly ascending sets N(v), total =
        sum over v, u in N(v) of |N(v) & N(u)| -- into the 64-bit word `total_buf`; `per_vertex_buf` (optional, get_num_rows()
        64-bit words) gets one credit for each of v, u, w per triple.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan
        keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, or its rows are no such sets
        (io.triangle_orient prepares them)."""
        if self.plan_ is None:
            _fatal("SpMVModule.tc_count: send_matrix_host_to_device first")
        self.plan_.tc_count(total_buf, per_vertex_buf)
        self._finish(total_buf, per_vertex_buf)

    def clique_count(self, k, total_buf, per_vertex_buf=None, stats=False):
        """Extension (gl_clique_count): the k-clique count, 3 <= k <= 8, of this module's matrix -- rows as strictly ascending
        sets N+(v), total = the sequences (v1 .. vk) with vj in N+(vi) for every i < j -- into the 64-bit word `total_buf`;
        `per_vertex_buf` (optional, get_num_rows() 64-bit words) gets one credit per position of every sequence.  stats=True ->
        (rows in the tiny and mid bins, rows in the wide bin, rows in the long bin, launches).  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, its
        rows are no such sets (io.orient_by_rank prepares them), or a row has more than 8192 entries (orient by a degeneracy
        rank); GL_ERR_INVALID_ARG for any other k."""
        if self.plan_ is None:
            _fatal("SpMVModule.clique_count: send_matrix_host_to_device first")
        out = self.plan_.clique_count(k, total_buf, per_vertex_buf, stats)
        self._finish(total_buf, per_vertex_buf)
        return out

    def kcore(self, core_buf, order_buf=None):
        """Extension (gl_kcore): the core numbers of this module's matrix, read as a graph -- rows as strictly ascending sets
        N(v), the pattern symmetric -- into `core_buf` (get_num_rows() words) and, optionally, a peeling order into `order_buf`
        -> (degeneracy, levels, sub-rounds, launches).  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when
        the plan keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, its rows are no such sets or
        its pattern is not symmetric (io.symmetrize_simple prepares it)."""
        if self.plan_ is None:
            _fatal("SpMVModule.kcore: send_matrix_host_to_device first")
        stats = self.plan_.kcore(core_buf, order_buf)
        self._finish(core_buf, order_buf)
        return stats

    def color(self, color_buf, prio_buf=None):
        """Extension (gl_color): the first-fit greedy colouring of this module's matrix, read as a graph -- rows as strictly
        ascending sets N(v), the pattern symmetric -- in the order of `prio_buf` (get_num_rows() words, larger first, ties by
        vertex number; None: ascending vertex order) into `color_buf` (get_num_rows() words) -> (num_colors, rounds, launches,
        widest).  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the
        (||,&&) layout does), is not square, is a row shard, its rows are no such sets or its pattern is not symmetric
        (io.symmetrize_simple prepares it)."""
        if self.plan_ is None:
            _fatal("SpMVModule.color: send_matrix_host_to_device first")
        stats = self.plan_.color(prio_buf, color_buf)
        self._finish(color_buf)
        return stats

    def truss(self, truss_buf, support_buf=None):
        """Extension (gl_truss): the truss number of every edge of this module's matrix, read as a graph -- rows as strictly
        ascending sets N(v), the pattern symmetric -- into `truss_buf` and, optionally, the triangles through it into
        `support_buf` (get_nnz() words each, aligned with the matrix's entries) -> (max_truss, levels, sub-rounds, launches,
        edges, triangles).  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy
        (only the (||,&&) layout does), is not square, is a row shard, its rows are no such sets or its pattern is not symmetric
        (io.symmetrize_simple prepares it)."""
        if self.plan_ is None:
            _fatal("SpMVModule.truss: send_matrix_host_to_device first")
        stats = self.plan_.truss(truss_buf, support_buf)
        self._finish(truss_buf, support_buf)
        return stats

    def msf(self, weight_buf, forest_buf, labels_buf=None):
        """Extension (gl_msf): the minimum spanning forest of this module's matrix, read as a graph -- rows as strictly ascending
        sets N(v), the pattern symmetric -- under the f32 weights in `weight_buf` (get_nnz() words aligned with the matrix's
        entries; only the words of entries above the diagonal are read), into `forest_buf` (as many words: 1 for the entries of
        forest edges) and, optionally, the components' smallest vertices into `labels_buf` (get_num_cols() words) -> (forest
        edges, components, rounds, launches).  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan
        keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, its rows are no such sets or its
        pattern is not symmetric (io.symmetrize_weighted prepares it)."""
        if self.plan_ is None:
            _fatal("SpMVModule.msf: send_matrix_host_to_device first")
        stats = self.plan_.msf(weight_buf, forest_buf, labels_buf)
        self._finish(forest_buf, labels_buf)
        return stats

    def match(self, weight_buf, mate_buf):
        """Extension (gl_match): the greedy weighted matching of this module's matrix, read as a graph -- rows as strictly
        ascending sets N(v), the pattern symmetric -- under the f32 weights in `weight_buf` (get_nnz() words aligned with the
        matrix's entries; both entries of an edge hold the same word), into `mate_buf` (get_num_cols() words: every vertex's
        partner, 0xffffffff for a free vertex) -> (matched edges, rounds, scans, launches).  The call synchronises.  Raises
        GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a
        row shard, its rows are no such sets or its pattern is not symmetric (io.symmetrize_weighted prepares it)."""
        if self.plan_ is None:
            _fatal("SpMVModule.match: send_matrix_host_to_device first")
        stats = self.plan_.match(weight_buf, mate_buf)
        self._finish(mate_buf)
        return stats

    def lpa(self, label_buf, color_buf=None, init_buf=None, max_sweeps=100):
        """Extension (gl_lpa): label propagation communities of this module's matrix, read as a graph -- rows as strictly
        ascending sets N(v), the pattern symmetric -- into `label_buf` (get_num_rows() words), from the initial labels in
        `init_buf` (as many words, none 0xffffffff; None: every vertex's own number), swept colour class by colour class under
        the proper colouring in `color_buf` (as many words; SpMVModule.color gives one), or synchronously with color_buf=None
        -> (sweeps, changes, evaluations, launches, converged).  The call synchronises.  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, its
        rows are no such sets or its pattern is not symmetric (io.symmetrize_simple prepares it), and (GL_ERR_INVALID_ARG) for
        a label 0xffffffff, a colour >= get_num_rows() or a colouring that is not proper."""
        if self.plan_ is None:
            _fatal("SpMVModule.lpa: send_matrix_host_to_device first")
        stats = self.plan_.lpa(label_buf, color_buf, init_buf, max_sweeps)
        self._finish(label_buf)
        return stats

    def louvain_move(self, label_buf, color_buf, weight_buf=None, vertex_weight_buf=None, max_sweeps=100, min_gain=0):
        """Extension (gl_louvain_move): one level of Louvain's local moving on this module's matrix, read as a graph -- rows as
        strictly ascending sets N(v), the pattern symmetric -- into `label_buf` (get_num_rows() words), swept colour class by
        colour class under the proper colouring in `color_buf` (as many words; SpMVModule.color gives one), under the integer
        entry weights in `weight_buf` (get_nnz() words aligned with the matrix's entries, each at least 1, both entries of an
        edge the same; None: all 1) and the vertex weights in `vertex_weight_buf` (get_num_rows() words; None: the sums of the
        entry weights) -> (sweeps, moves, evaluations, launches, stop reason, q_first, q_last).  The call synchronises.  Raises
        GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a
        row shard, its rows are no such sets, its pattern is not symmetric (io.symmetrize_simple prepares it) or the vertex
        weights sum to 2^31 or more, and (GL_ERR_INVALID_ARG) for a colour >= get_num_rows(), a colouring that is not proper, a
        zero weight or a vertex weight below its entries' sum."""
        if self.plan_ is None:
            _fatal("SpMVModule.louvain_move: send_matrix_host_to_device first")
        stats = self.plan_.louvain_move(label_buf, color_buf, weight_buf, vertex_weight_buf, max_sweeps, min_gain)
        self._finish(label_buf)
        return stats

    def contract(self, label_buf, num_vertices=None, weight_buf=None, vertex_weight_buf=None):
        """Extension (gl_contract_symbolic + gl_contract_numeric): the quotient of this module's matrix, read as a graph -- rows as
        strictly ascending sets, directed or not --, by the labelling in `label_buf` (num_vertices words, default
        get_num_rows(); every label a vertex number below num_vertices), under the uint32 entry weights in `weight_buf`
        (get_nnz() words aligned with the matrix's entries; None: all 1) and the vertex weights in `vertex_weight_buf` (None: the
        sums of the rows' entry weights) -> (io.CSRMatrix of the k groups, uint32 weights, uint32 tot, uint32 part, stats): on
        the host, io.aggregate_communities' tuple and gl_contract_numeric's six figures.  The groups are numbered in ascending
        order of their labels.  The call synchronises; only C, tot and part cross to the host.  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, its
        rows are no such sets or a row at or behind num_vertices is not empty, and (GL_ERR_INVALID_ARG) for a label >=
        num_vertices."""
        if self.plan_ is None:
            _fatal("SpMVModule.contract: send_matrix_host_to_device first")
        nv = self.get_num_rows() if num_vertices is None else int(num_vertices)
        head = capi.DeviceBuffer(4 * (2 * nv + 1 + 1))                     # (32-bit words: part, then the offsets of C)
        part_buf = capi.DeviceBuffer(4 * max(nv, 1), ptr=head.ptr, keepalive=head)
        indptr_buf = capi.DeviceBuffer(4 * (nv + 1), ptr=head.ptr + 4 * max(nv, 1), keepalive=head)
        k, nnz = self.plan_.contract_symbolic(nv, label_buf, part_buf, indptr_buf)[:2]
        body = capi.DeviceBuffer(4 * (2 * nnz + k + 1))                    # (the columns, the weights, tot)
        idx_buf = capi.DeviceBuffer(4 * max(nnz, 1), ptr=body.ptr, keepalive=body)
        w_buf = capi.DeviceBuffer(4 * max(nnz, 1), ptr=body.ptr + 4 * nnz, keepalive=body)
        tot_buf = capi.DeviceBuffer(4 * max(k, 1), ptr=body.ptr + 8 * nnz, keepalive=body)
        stats = self.plan_.contract_numeric(nv, part_buf, k, indptr_buf, idx_buf, w_buf, tot_buf, weight_buf, vertex_weight_buf, stats=True)
        words = head.read(np.uint32, 2 * nv + 1 + 1)
        part, indptr = words[:nv], words[max(nv, 1):max(nv, 1) + k + 1]
        out = body.read(np.uint32, 2 * nnz + k + 1)
        from .io import CSRMatrix
        c = CSRMatrix(k, k, np.ones(nnz, dtype=np.float32), out[:nnz].copy(), indptr.copy())
        return c, out[nnz:2 * nnz].copy(), out[2 * nnz:2 * nnz + k].copy(), part.copy(), stats

    def scc(self, out_module, label_buf, prio_buf=None):
        """Extension (gl_scc): the strongly connected components of this module's matrix, read as a directed graph -- row v: the
        predecessors of v, `out_module` (None: the pattern is symmetric) holds the transposed pattern -- into `label_buf`
        (get_num_rows() words: the smallest vertex of every vertex's component) -> (components, passes, trimmed, rounds,
        launches).  `prio_buf` (as many words, larger first, ties by vertex number; None: all equal) decides which component a
        pass removes, never the labels.  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when a plan keeps no
        row copy (only the (||,&&) layout does), is not square, is a row shard, its rows are no strictly ascending sets, or the
        two are not each other's transpose (io.simple_pattern prepares them)."""
        if self.plan_ is None or (out_module is not None and out_module.plan_ is None):
            _fatal("SpMVModule.scc: send_matrix_host_to_device first")
        stats = self.plan_.scc(None if out_module is None else out_module.plan_, label_buf, prio_buf)
        self._finish(label_buf)
        return stats

    def bicc(self, block_buf, vertex_blocks_buf=None, edge_component_buf=None, tree_buf=None):
        """Extension (gl_bicc): the biconnected components of this module's matrix, read as an undirected simple graph -- rows as
        strictly ascending sets N(v), the pattern symmetric -- into `block_buf` (get_nnz() words, aligned with the matrix's
        entries: the smallest entry number of the block of every entry's edge) and, optionally, `vertex_blocks_buf` (the blocks
        a vertex belongs to; >= 2: an articulation point), `edge_component_buf` (the smallest vertex of its 2-edge-connected
        component; get_num_rows() words each) and `tree_buf` (6 get_num_rows() words: level, parent, pre, nd, low, high) ->
        (blocks, articulation points, bridges, depth, launches, trees).  The call synchronises.  Raises GraphLilyError
        (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not square, is a row shard, or
        its rows are no strictly ascending sets or its pattern is not symmetric (io.symmetrize_simple prepares the matrix)."""
        if self.plan_ is None:
            _fatal("SpMVModule.bicc: send_matrix_host_to_device first")
        stats = self.plan_.bicc(block_buf, vertex_blocks_buf, edge_component_buf, tree_buf)
        self._finish(block_buf, vertex_blocks_buf, edge_component_buf, tree_buf)
        return stats

    def topo(self, out_module, level_buf, order_buf=None, weight_buf=None, dist_buf=None, parent_buf=None):
        """Extension (gl_topo): the topological levels of this module's matrix, read as a directed graph -- row v: the
        predecessors of v, `out_module` (None: the pattern is symmetric) holds the transposed pattern -- into `level_buf`
        (get_num_rows() words: the edges of the longest path that ends in v, 0xffffffff on a cycle or behind one) -> (peeled,
        levels, widest, launches).  `order_buf` (optional, as many words) receives the peeled vertices grouped by level.  With
        `weight_buf` (get_nnz() floats aligned with the matrix's entries, finite) `dist_buf` and `parent_buf` (get_num_rows()
        words each) receive the weighted longest path and its predecessor tree (ties to the smallest predecessor).  The call
        synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when a plan keeps no row copy (only the (||,&&) layout does),
        is not square, is a row shard, its rows are no strictly ascending sets, or the two are not each other's transpose
        (io.directed_weighted prepares them)."""
        if self.plan_ is None or (out_module is not None and out_module.plan_ is None):
            _fatal("SpMVModule.topo: send_matrix_host_to_device first")
        stats = self.plan_.topo(None if out_module is None else out_module.plan_, level_buf, order_buf, weight_buf, dist_buf, parent_buf)
        self._finish(level_buf, order_buf, dist_buf, parent_buf)
        return stats

    def sssp_delta(self, out_module, weight_buf, weight_out_buf, sources, delta, dist_buf, parent_buf=None):
        """Extension (gl_sssp_delta): delta-stepping shortest paths over this module's matrix, read as a directed graph -- row v:
        the predecessors of v, `out_module` (None: the pattern is symmetric) holds the transposed pattern -- from `sources`
        (host vertex numbers, all at distance 0) into `dist_buf` (get_num_rows() floats: Dijkstra's f32 result to the bit,
        whatever `delta`, a float > 0 or +inf; the bits 0x7f800000 when unreached) -> (reached, buckets, rounds, relaxations,
        launches).  `weight_buf` and `weight_out_buf` (get_nnz() floats each, finite and >= +0.0) are aligned with this
        matrix's entries and with out_module's.  `parent_buf` (optional, get_num_rows() words) receives the predecessor tree,
        ties to the smallest predecessor.  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when a plan keeps
        no row copy (only the (||,&&) layout does), is not square, is a row shard, its rows are no strictly ascending sets, or
        the two are not each other's transpose (io.directed_weighted prepares them)."""
        if self.plan_ is None or (out_module is not None and out_module.plan_ is None):
            _fatal("SpMVModule.sssp_delta: send_matrix_host_to_device first")
        stats = self.plan_.sssp_delta(None if out_module is None else out_module.plan_, weight_buf, weight_out_buf, sources, delta, dist_buf,
                                      parent_buf)
        self._finish(dist_buf, parent_buf)
        return stats

    def msbfs(self, sources, far_buf, reach_buf, harmonic_buf, accumulate=False, hops_buf=None):
        """Extension (gl_msbfs): the bit-parallel breadth-first search from up to 64 `sources` (host vertex numbers) over this
        module's matrix, read as a directed graph -- row v: the predecessors of v, so the distances run FROM the sources; the
        transposed pattern's module measures them TO the sources -- -> (source_stats, stats): uint64[k, 3] of {vertices at
        distance >= 1, the sum of those distances, the eccentricity} per source, and (levels, vertices that met every source,
        launches, 0).  `far_buf` (get_num_rows() 64-bit words), `reach_buf` (as many words) and `harmonic_buf` (as many
        doubles) receive per vertex the sum and the number of its finite distances >= 1 and the sum of their reciprocals, or
        are added to with accumulate=True; `hops_buf` (optional, k * get_num_rows() words) receives the distances themselves,
        0xffffffff when unreached.  The call synchronises.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no
        row copy (only the (||,&&) layout does), is not square or is a row shard; the rows may hold anything."""
        if self.plan_ is None:
            _fatal("SpMVModule.msbfs: send_matrix_host_to_device first")
        out = self.plan_.msbfs(sources, far_buf, reach_buf, harmonic_buf, accumulate, hops_buf)
        self._finish(far_buf, reach_buf, harmonic_buf, hops_buf)
        return out

    def similarity(self, pairs_buf, common_buf, weighted_buf=None, vertex_weight_buf=None, stats=False, count=None):
        """Extension (gl_similarity): common_buf[i] = the number of common neighbours of the pair (u_i, v_i) of `pairs_buf` (2 m
        words u0 v0 u1 v1 ...; `count` = m, by default what the buffer holds) in this module's matrix, whose rows are read as
        sets -- io.symmetrize_simple / io.simple_pattern prepare it; on a directed pattern the common predecessors.
        `weighted_buf` (optional, m 64-bit words) receives the sum of `vertex_weight_buf` (get_num_rows() 64-bit unsigned
        words) over the common neighbours, modulo 2^64.  The pairs need not be edges; a vertex >= get_num_rows() gives
        0xffffffff and 0.  stats=False only enqueues; stats=True waits -> (pairs out of range, deferred pairs, launches, 0).
        Raises GraphLilyError (GL_ERR_UNSUPPORTED) when the plan keeps no row copy (only the (||,&&) layout does), is not
        square, is a row shard, or its rows are not strictly ascending sets."""
        if self.plan_ is None:
            _fatal("SpMVModule.similarity: send_matrix_host_to_device first")
        out = self.plan_.similarity(pairs_buf, common_buf, weighted_buf, vertex_weight_buf, stats, count)
        self._finish(common_buf, weighted_buf)
        return out

    def bc_accumulate(self, out_module, level_buf, bc_buf, scale=1.0, accumulate=False, sigma_buf=None, stats=True):
        """Extension (gl_bc_accumulate): adds scale x Brandes' dependency of the search whose levels are in `level_buf`
        (get_num_rows() floats) to `bc_buf` (as many doubles; accumulate=False: overwrites it).  This module's matrix is the
        pulling side (row v: the vertices v is pulled from), `out_module` (None: the pattern is symmetric) holds the transposed
        pattern.  `sigma_buf` (optional, doubles) receives the path counts.  -> (depth, reached, orphans, non-finite sigmas),
        or None with stats=False.  Raises GraphLilyError (GL_ERR_UNSUPPORTED) when a plan keeps no row copy (only the (||,&&)
        layout does), is not square, is a row shard, its rows are no strictly ascending sets, or the two are not each other's
        transpose (io.simple_pattern prepares them)."""
        if self.plan_ is None or (out_module is not None and out_module.plan_ is None):
            _fatal("SpMVModule.bc_accumulate: send_matrix_host_to_device first")
        st = self.plan_.bc_accumulate(None if out_module is None else out_module.plan_, level_buf, bc_buf, scale, accumulate, sigma_buf, stats)
        self._finish(bc_buf, sigma_buf)
        return st

    def fused_bfs_ok(self):
        if self.plan_ is None or not self._plan_serves(self.semiring_.op) or self.semiring_.zero != 0.0:
            return False
        info = self.plan_.info()
        return info["layout"] == "boolean" and info["segments"] == 1 and self.row_begin_ % 64 == 0

    def run_bits(self, bits_buf):
        mask = self.mask_buf if self.mask_type_ != kNoMask else None
        self.plan_.run_bits(bits_buf, mask, self.results_buf, self.semiring_.zero, self.mask_type_)
        self._finish(self.results_buf)

    def send_vector_device_to_host(self):
        return self.vector_buf.read(np.float32, self.get_num_cols())

    def send_mask_device_to_host(self):
        return self.mask_buf.read(np.float32, self.get_num_rows())

    def send_results_device_to_host(self):
        return self.results_buf.read(np.float32, self.get_num_rows())


class SpGEMMModule(BaseModule):
    """Extension (gl_spgemm_symbolic / gl_spgemm_numeric): C = A (+).(x) B with a sparse result, under the three
    semirings, with an optional structural mask.  The interface mirrors SpMVModule's.  A, B and the mask are square matrices over
    the same vertices.  The plans are boolean plans of all-ones values -- a zero VALUE is a legitimate value here, and the row
    copy would store it as no entry -- and the values travel in buffers of their own, in the order of the sorted rows."""

    def __init__(self):
        super().__init__()
        self.semiring_ = ArithmeticSemiring
        self.mask_type_ = kNoMask
        self.mask_slot_ = 0
        self.a_ = self.b_ = None                                   # host CSRs, rows strictly ascending
        self.masks_, self.plan_masks_ = {}, {}                     # by slot
        self.plan_a_ = self.plan_b_ = None
        self.a_val_buf = self.b_val_buf = None
        self.c_indptr_buf = self.c_indices_buf = self.c_val_buf = None
        self.nnz_ = 0
        self.stats_ = None

    def set_semiring(self, semiring):
        self.semiring_ = semiring

    def set_mask_type(self, mask_type, slot=0):
        """kNoMask; kMaskWriteToOne: C is written where the matrix of load_mask_matrix(csr, slot) stores an entry;
        kMaskWriteToZero: where it stores none (the complement) -- SpMVModule's reading of the two, with "stored" for
        "non-zero"."""
        assert mask_type in (kNoMask, kMaskWriteToZero, kMaskWriteToOne)
        self.mask_type_, self.mask_slot_ = mask_type, slot

    @staticmethod
    def _sorted_rows(csr, who):
        """-> the square matrix with the columns of every row ascending, the values carried along; duplicates are refused"""
        n = int(csr.num_rows)
        if n != int(csr.num_cols):
            raise ValueError("SpGEMMModule.%s: a %d x %d matrix: rectangular operands are out of scope" % (who, n, int(csr.num_cols)))
        indptr = np.asarray(csr.adj_indptr).astype(np.int64)[:n + 1]
        nnz = int(indptr[-1])
        key = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) * n + np.asarray(csr.adj_indices[:nnz]).astype(np.int64)
        order = np.argsort(key, kind="stable")
        key = key[order]
        if np.any(key[1:] == key[:-1]):
            j = int(np.flatnonzero(key[1:] == key[:-1])[0])
            raise ValueError("SpGEMMModule.%s: entry (%d, %d) is stored twice" % (who, key[j] // n, key[j] % n))
        return type(csr)(n, n, np.asarray(csr.adj_data[:nnz], dtype=np.float32)[order], (key % max(n, 1)).astype(np.uint32), indptr.astype(np.uint32))

    def get_num_rows(self):
        return self.a_.num_rows

    def load_and_format_matrices(self, a_csr, b_csr=None):
        """b_csr=None: C = A (+).(x) A on one plan"""
        self.a_ = self._sorted_rows(a_csr, "load_and_format_matrices")
        self.b_ = self.a_ if b_csr is None else self._sorted_rows(b_csr, "load_and_format_matrices")
        if self.b_.num_rows != self.a_.num_rows:
            raise ValueError("SpGEMMModule.load_and_format_matrices: %d and %d vertices" % (self.a_.num_rows, self.b_.num_rows))

    def load_mask_matrix(self, csr, slot=0):
        """several masks may be loaded, one per slot: they share the plans of A and B"""
        self.masks_[slot] = self._sorted_rows(csr, "load_mask_matrix")

    @staticmethod
    def _ones_plan(m):
        return capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, np.ones(m.adj_indices.shape[0], dtype=np.float32), 0,
                             m.num_rows, capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD)

    def send_matrices_host_to_device(self):
        self.plan_a_ = self._ones_plan(self.a_)
        self.a_val_buf = capi.DeviceBuffer.from_host(self.a_.adj_data if self.a_.adj_data.shape[0] else np.zeros(1, np.float32))
        if self.b_ is self.a_:
            self.plan_b_, self.b_val_buf = self.plan_a_, self.a_val_buf
        else:
            self.plan_b_ = self._ones_plan(self.b_)
            self.b_val_buf = capi.DeviceBuffer.from_host(self.b_.adj_data if self.b_.adj_data.shape[0] else np.zeros(1, np.float32))
        self.plan_masks_ = {}
        for slot, mask in self.masks_.items():
            if mask.num_rows != self.a_.num_rows:
                raise ValueError("SpGEMMModule: a mask is over %d vertices, the operands over %d" % (mask.num_rows, self.a_.num_rows))
            self.plan_masks_[slot] = self._ones_plan(mask)
        self._finish(self.a_val_buf, self.b_val_buf)

    def run(self):
        """symbolic, then the buffers of C, then numeric.  Leaves nnz_ and stats_ = (nnz(C), products, rows that took the
        workgroup path, rows that took the slab path) of the symbolic call.  NaN values are refused under every semiring,
        +-inf under (+,x) (ValueError)."""
        if self.plan_a_ is None:
            _fatal("SpGEMMModule.run: send_matrices_host_to_device first")
        op = self.semiring_.op
        for name, m in (("A", self.a_), ("B", self.b_)):
            if op != kLogicalAndOr and (np.isnan(m.adj_data).any() or (op == kMulAdd and np.isinf(m.adj_data).any())):
                raise ValueError("SpGEMMModule.run: %s holds a NaN%s value" % (name, " or an infinite" if op == kMulAdd else ""))
        mask = None
        if self.mask_type_ != kNoMask:
            if self.mask_slot_ not in self.plan_masks_:
                _fatal("SpGEMMModule.run: load_mask_matrix before send_matrices_host_to_device")
            mask = self.plan_masks_[self.mask_slot_]
        complement = self.mask_type_ == kMaskWriteToZero
        n = self.a_.num_rows
        self.c_indptr_buf = capi.DeviceBuffer(4 * (n + 1))
        self.stats_ = self.plan_a_.spgemm_symbolic(self.plan_b_, self.c_indptr_buf, mask, complement)
        self.nnz_ = self.stats_[0]
        self.c_indices_buf = capi.DeviceBuffer(4 * max(1, self.nnz_))
        self.c_val_buf = capi.DeviceBuffer(4 * max(1, self.nnz_))
        self.plan_a_.spgemm_numeric(self.plan_b_, op, self.a_val_buf, self.b_val_buf, self.c_indptr_buf, self.c_indices_buf, self.c_val_buf,
                                    mask, complement)
        self._finish(self.c_indptr_buf, self.c_indices_buf, self.c_val_buf)

    def send_results_device_to_host(self):
        """-> io.CSRMatrix: C, the columns of every row ascending; under (||,&&) every value is 1"""
        from . import io
        n = self.a_.num_rows
        return io.CSRMatrix(n, n, self.c_val_buf.read(np.float32, self.nnz_), self.c_indices_buf.read(np.uint32, self.nnz_),
                            self.c_indptr_buf.read(np.uint32, n + 1))


class SpMMModule(BaseModule):
    """Extension (gl_spmm): Y = A (+).(x) X for a dense block X of k vectors, under the three semirings, with an
    optional dense mask of Y's shape -- one pass over A where k SpMVModule runs make k.  The interface mirrors SpMVModule's; X is
    an (num_cols, k) array, Y and the mask are (num_rows, k), all row-major.  A may be rectangular and a row shard.  The plan is a
    boolean plan of all-ones values -- a zero VALUE is a value here, and the row copy would store it as no entry -- and the
    values travel in a buffer of their own, in the matrix' order."""

    def __init__(self):
        super().__init__()
        self.semiring_ = ArithmeticSemiring
        self.mask_type_ = kNoMask
        self.csr_matrix_ = None
        self.plan_ = None
        self.row_begin_, self.row_end_ = 0, None
        self.k_ = 0
        self.ldx_ = self.ldy_ = self.ldm_ = None               # leading dimensions of bound buffers (None: k)
        self.vectors_nan_ = self.vectors_inf_ = False          # of the X that send_vectors_host_to_device saw
        self.a_val_buf = self.vectors_buf = self.mask_buf = self.results_buf = None
        self.stats_ = None

    def set_semiring(self, semiring):
        self.semiring_ = semiring

    def set_mask_type(self, mask_type):
        assert mask_type in (kNoMask, kMaskWriteToZero, kMaskWriteToOne)
        self.mask_type_ = mask_type

    def set_row_shard(self, row_begin, row_end):
        """this device owns rows [row_begin, row_end) of the matrix: only those rows of Y are written"""
        self.row_begin_, self.row_end_ = int(row_begin), int(row_end)

    def get_num_rows(self):
        return self.csr_matrix_.num_rows

    def get_num_cols(self):
        return self.csr_matrix_.num_cols

    def get_num_vectors(self):
        return self.k_

    def load_and_format_matrix(self, csr_matrix_float):
        self.csr_matrix_ = csr_matrix_float

    def send_matrix_host_to_device(self):
        m = self.csr_matrix_
        r0, r1 = self.row_begin_, m.num_rows if self.row_end_ is None else self.row_end_
        indptr = np.asarray(m.adj_indptr).astype(np.int64)
        nnz = int(indptr[m.num_rows])
        self.plan_ = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, np.ones(nnz, dtype=np.float32), r0, r1,
                                   capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD)
        self.values_ = np.ascontiguousarray(m.adj_data[int(indptr[r0]):int(indptr[r1])], dtype=np.float32)   # the shard's entries
        self.a_val_buf = capi.DeviceBuffer.from_host(self.values_ if self.values_.shape[0] else np.zeros(1, np.float32))
        self._finish(self.a_val_buf)

    def send_vectors_host_to_device(self, vectors):
        """X: an (num_cols, k) array; k is taken from it.  Allocates the results buffer for that k (zero-filled) unless one of that
        size is there."""
        x = np.ascontiguousarray(vectors, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.get_num_cols() or x.shape[1] == 0:
            raise ValueError("SpMMModule.send_vectors_host_to_device: X must be (%d, k >= 1), got %s" % (self.get_num_cols(), x.shape))
        self.k_, self.ldx_ = int(x.shape[1]), None
        self.vectors_nan_, self.vectors_inf_ = bool(np.isnan(x).any()), bool(np.isinf(x).any())
        self.vectors_buf = capi.DeviceBuffer.from_host(x)
        if self.results_buf is None or self.ldy_ is not None or self.results_buf.nbytes != 4 * self.get_num_rows() * self.k_:
            self.results_buf, self.ldy_ = capi.DeviceBuffer(4 * max(1, self.get_num_rows() * self.k_)), None
            capi.fill_f32(self.results_buf, 0.0, self.get_num_rows() * self.k_)
        self._finish(self.vectors_buf, self.results_buf)

    def send_mask_host_to_device(self, mask):
        """M: an (num_rows, k) array"""
        m = np.ascontiguousarray(mask, dtype=np.float32)
        if m.shape != (self.get_num_rows(), self.k_):
            raise ValueError("SpMMModule.send_mask_host_to_device: the mask must be %s, got %s" % ((self.get_num_rows(), self.k_), m.shape))
        self.mask_buf, self.ldm_ = capi.DeviceBuffer.from_host(m if m.size else np.zeros(1, np.float32)), None
        self._finish(self.mask_buf)

    def bind_vectors_buf(self, src_buf, k, ld=None):
        """a device block of num_cols x k floats with the leading dimension `ld` (None: k); its contents are the caller's business"""
        self.vectors_buf, self.k_, self.ldx_ = src_buf, int(k), ld
        self.vectors_nan_ = self.vectors_inf_ = False

    def bind_mask_buf(self, src_buf, ld=None):
        self.mask_buf, self.ldm_ = src_buf, ld

    def bind_results_buf(self, src_buf, ld=None):
        self.results_buf, self.ldy_ = src_buf, ld

    def run(self):
        """Leaves stats_ = (rows on the short path, rows on the wavefront path, rows on the workgroup path, column tiles).  NaN
        values are refused under every semiring, +-inf under (+,x) (ValueError): of A, and of an X this module uploaded."""
        if self.plan_ is None or self.vectors_buf is None:
            _fatal("SpMMModule.run: send_matrix_host_to_device and send_vectors_host_to_device first")
        op = self.semiring_.op
        if op != kLogicalAndOr and (np.isnan(self.values_).any() or self.vectors_nan_ or
                                    (op == kMulAdd and (np.isinf(self.values_).any() or self.vectors_inf_))):
            raise ValueError("SpMMModule.run: A or X holds a NaN%s value" % (" or an infinite" if op == kMulAdd else ""))
        mask = self.mask_buf if self.mask_type_ != kNoMask else None
        if self.mask_type_ != kNoMask and mask is None:
            _fatal("SpMMModule.run: a mask type without a mask")
        self.stats_ = self.plan_.spmm(None if op == kLogicalAndOr else self.a_val_buf, self.vectors_buf, self.results_buf, self.k_, op,
                                      self.semiring_.zero, mask, self.mask_type_, self.ldx_, self.ldy_, self.ldm_, stats=True)
        self._finish(self.results_buf)

    def send_results_device_to_host(self):
        """-> an (num_rows, k) array (of a bound buffer with a leading dimension: its k columns)"""
        n, ld = self.get_num_rows(), self.k_ if self.ldy_ is None else self.ldy_
        if n == 0:
            return np.zeros((0, self.k_), np.float32)
        flat = self.results_buf.read(np.float32, (n - 1) * ld + self.k_)
        return np.ascontiguousarray(np.lib.stride_tricks.as_strided(flat, (n, self.k_), (4 * ld, 4)))


class SDDMMModule(BaseModule):
    """Extension (gl_sddmm): C = A (x) (X (+).(x) Y^T) sampled at A's entries -- one score per stored entry of A from
    the k features of its row (X, (num_rows, k)) and of its column (Y, (num_cols, k)), under the three semirings; the edge half of
    a message-passing layer, of which SpMMModule is the aggregating half.  The interface mirrors SpMMModule's.  A may be
    rectangular and a row shard.  results_buf is the plain per-entry buffer (an f32 per entry of the shard's rows, in the matrix'
    order): it can be handed to SpMMModule as its a_val_buf as it is."""

    def __init__(self):
        super().__init__()
        self.semiring_ = ArithmeticSemiring
        self.scaled_ = True
        self.csr_matrix_ = None
        self.plan_ = None
        self.row_begin_, self.row_end_ = 0, None
        self.k_ = 0
        self.ldx_ = self.ldy_ = None                           # leading dimensions of bound buffers (None: k)
        self.features_nan_ = self.features_inf_ = False        # of the X and Y that send_features_host_to_device saw
        self.a_val_buf = self.x_buf = self.y_buf = self.results_buf = None
        self.stats_ = None

    def set_semiring(self, semiring):
        self.semiring_ = semiring

    def set_scaled(self, scaled):
        """True (the default): the scores are scaled by A's values; False: the bracket itself, A gives the pattern only"""
        self.scaled_ = bool(scaled)

    def set_row_shard(self, row_begin, row_end):
        """this device owns rows [row_begin, row_end) of the matrix: only those rows' entries are scored"""
        self.row_begin_, self.row_end_ = int(row_begin), int(row_end)

    def get_num_rows(self):
        return self.csr_matrix_.num_rows

    def get_num_cols(self):
        return self.csr_matrix_.num_cols

    def get_num_features(self):
        return self.k_

    def load_and_format_matrix(self, csr_matrix_float):
        self.csr_matrix_ = csr_matrix_float

    def send_matrix_host_to_device(self):
        """Allocates the results buffer, an f32 per entry of the shard's rows (zero-filled)"""
        m = self.csr_matrix_
        r0, r1 = self.row_begin_, m.num_rows if self.row_end_ is None else self.row_end_
        indptr = np.asarray(m.adj_indptr).astype(np.int64)
        nnz = int(indptr[m.num_rows])
        self.plan_ = capi.SpMVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, np.ones(nnz, dtype=np.float32), r0, r1,
                                   capi.GL_PLAN_BOOLEAN | capi.GL_PLAN_NO_MULADD)
        self.first_, self.count_ = int(indptr[r0]), int(indptr[r1] - indptr[r0])
        self.values_ = np.ascontiguousarray(m.adj_data[self.first_:self.first_ + self.count_], dtype=np.float32)   # the shard's entries
        self.a_val_buf = capi.DeviceBuffer.from_host(self.values_ if self.count_ else np.zeros(1, np.float32))
        self.results_buf = capi.DeviceBuffer(4 * max(1, self.count_))
        if self.count_:
            capi.fill_f32(self.results_buf, 0.0, self.count_)
        self._finish(self.a_val_buf, self.results_buf)

    def send_features_host_to_device(self, X, Y):
        """X: an (num_rows, k) array, Y: an (num_cols, k) array; k is taken from them"""
        x, y = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Y, dtype=np.float32)
        if x.ndim != 2 or y.ndim != 2 or x.shape[0] != self.get_num_rows() or y.shape[0] != self.get_num_cols() or x.shape[1] != y.shape[1] or x.shape[1] == 0:
            raise ValueError("SDDMMModule.send_features_host_to_device: X must be (%d, k) and Y (%d, k), k >= 1, got %s and %s" %
                             (self.get_num_rows(), self.get_num_cols(), x.shape, y.shape))
        self.k_, self.ldx_, self.ldy_ = int(x.shape[1]), None, None
        self.features_nan_ = bool(np.isnan(x).any() or np.isnan(y).any())
        self.features_inf_ = bool(np.isinf(x).any() or np.isinf(y).any())
        self.x_buf = capi.DeviceBuffer.from_host(x if x.size else np.zeros(1, np.float32))
        self.y_buf = capi.DeviceBuffer.from_host(y if y.size else np.zeros(1, np.float32))
        self._finish(self.x_buf, self.y_buf)

    def bind_features_bufs(self, x_buf, y_buf, k, ldx=None, ldy=None):
        """device blocks of num_rows x k and num_cols x k floats with the leading dimensions ldx, ldy (None: k); their contents
        are the caller's business"""
        self.x_buf, self.y_buf, self.k_, self.ldx_, self.ldy_ = x_buf, y_buf, int(k), ldx, ldy
        self.features_nan_ = self.features_inf_ = False

    def bind_results_buf(self, src_buf):
        """a device buffer of an f32 per entry of the shard's rows"""
        self.results_buf = src_buf

    def run(self):
        """Leaves stats_ = (rows on the short path, pieces on the piece path, feature tiles).  NaN values are refused under every
        semiring, +-inf under (+,x) (ValueError): of A when its values scale, and of an X and Y this module uploaded."""
        if self.plan_ is None or self.x_buf is None:
            _fatal("SDDMMModule.run: send_matrix_host_to_device and send_features_host_to_device first")
        op = self.semiring_.op
        scaled = self.scaled_ and op != kLogicalAndOr
        if op != kLogicalAndOr and ((scaled and np.isnan(self.values_).any()) or self.features_nan_ or
                                    (op == kMulAdd and ((scaled and np.isinf(self.values_).any()) or self.features_inf_))):
            raise ValueError("SDDMMModule.run: A, X or Y holds a NaN%s value" % (" or an infinite" if op == kMulAdd else ""))
        self.stats_ = self.plan_.sddmm(self.a_val_buf if scaled else None, self.x_buf, self.y_buf, self.results_buf, self.k_, op,
                                       self.semiring_.zero, self.ldx_, self.ldy_, stats=True)
        self._finish(self.results_buf)

    def send_results_device_to_host(self):
        """-> an io.CSRMatrix with A's pattern and the scores as values: the shard's rows filled, the others empty"""
        from . import io
        m = self.csr_matrix_
        r0, r1 = self.row_begin_, m.num_rows if self.row_end_ is None else self.row_end_
        indptr = np.asarray(m.adj_indptr).astype(np.int64)[:m.num_rows + 1]
        out_ptr = np.clip(indptr, indptr[r0], indptr[r1]) - indptr[r0]
        scores = self.results_buf.read(np.float32, self.count_) if self.count_ else np.zeros(0, np.float32)
        return io.CSRMatrix(m.num_rows, m.num_cols, scores, np.asarray(m.adj_indices[self.first_:self.first_ + self.count_]).astype(np.uint32),
                            out_ptr.astype(np.uint32))


class SpMSpVModule(BaseModule):
    def __init__(self, out_buf_len=0):
        super().__init__()
        self.out_buf_len_ = out_buf_len
        self.mask_type_ = kNoMask
        self.semiring_ = ArithmeticSemiring
        self.csc_matrix_ = None
        self.plan_ = None
        self.row_begin_, self.row_end_ = 0, None
        self.vector_buf = self.mask_buf = self.results_buf = None

    def set_semiring(self, semiring):
        self.semiring_ = semiring

    def set_mask_type(self, mask_type):
        self.mask_type_ = mask_type

    def set_row_shard(self, row_begin, row_end):
        self.row_begin_, self.row_end_ = int(row_begin), int(row_end)

    def get_num_rows(self):
        return self.csc_matrix_.num_rows

    def get_num_cols(self):
        return self.csc_matrix_.num_cols

    def get_nnz(self):
        return int(self.csc_matrix_.adj_indptr[self.csc_matrix_.num_cols])

    def load_and_format_matrix(self, csc_matrix_float):
        self.csc_matrix_ = csc_matrix_float

    def send_matrix_host_to_device(self):
        m = self.csc_matrix_
        re = m.num_rows if self.row_end_ is None else self.row_end_
        self.plan_ = capi.SpMSpVPlan(m.num_rows, m.num_cols, m.adj_indptr, m.adj_indices, m.adj_data,
                                     self.row_begin_, re)
        # results: num_rows + 1 sparse elements, zero-initialised (spmspv_module.h:283-285)
        self.results_buf = capi.DeviceBuffer(8 * (m.num_rows + 1))
        self.results_buf.write(np.zeros(m.num_rows + 1, dtype=IDX_VAL))

        self._attach(getattr(self, "pull_module_", None))

    def attach_pull(self, spmv_module):
        """Extension (no counterpart in the reference): let heavy (||,&&) frontiers run row-wise on the boolean
        plan of an SpMVModule that holds the same matrix and row shard (gl_spmspv_plan_attach_pull)."""
        self.pull_module_ = spmv_module
        if not hasattr(spmv_module, "pull_clients_"):
            spmv_module.pull_clients_ = []
        if self not in spmv_module.pull_clients_:
            spmv_module.pull_clients_.append(self)
        self._attach(spmv_module)

    def sssp_parents(self, distance_buf, unreached, source, parent_buf, orphans_buf=None):
        """Extension (gl_sssp_parents): the shortest-path predecessor tree of the distance vector in `distance_buf`
        (get_num_cols() floats, `unreached` = the semiring's zero) from `source`, for this module's rows, into `parent_buf`
        (uint32 words; 0xffffffff = none).  One pass over the CSC this module's plan keeps."""
        if self.plan_ is None:
            _fatal("SpMSpVModule.sssp_parents: send_matrix_host_to_device first")
        self.plan_.sssp_parents(distance_buf, unreached, source, parent_buf, orphans_buf)
        self._finish(parent_buf)

    def hint_vector_nnz(self, nnz):
        """Extension: the caller knows the next run's vector holds at most `nnz` entries (gl_spmspv_plan_hint)."""
        if self.plan_ is not None:
            self.plan_.hint(nnz)

    def _attach(self, spmv_module):
        if self.plan_ is None:
            return
        plan = getattr(spmv_module, "plan_", None) if spmv_module is not None else None
        self.plan_.attach_pull(None)
        if plan is None:
            return
        mine = self.plan_
        if (plan.num_rows, plan.num_cols, plan.row_begin, plan.row_end) != (mine.num_rows, mine.num_cols, mine.row_begin, mine.row_end):
            return      # the SpMV module already holds the next matrix; this module attaches when its own is sent
        # boolean layout -> serves (||,&&); general / pattern layout -> (min,+) and, unless GL_PLAN_NO_MULADD, (+,x)
        self.plan_.attach_pull(plan)

    def enable_own_pull(self):
        """Extension for stand-alone use (no SpMVModule around, e.g. the bench_spmspv sweep): build a row-wise plan of
        this module's own matrix for its current semiring and attach it.  Costs a second formatted copy of the matrix."""
        from . import io as _io
        c = self.csc_matrix_
        # the CSC arrays of A are the CSR arrays of A^T; transposing that once more gives A by rows
        at = _io.CSRMatrix(c.num_cols, c.num_rows, c.adj_data, c.adj_indices, c.adj_indptr)
        a = _io.csr2csc(at)
        csr = _io.CSRMatrix(c.num_rows, c.num_cols, a.adj_data, a.adj_indices, a.adj_indptr)
        own = SpMVModule(num_hbm_channels, 0, 0)
        own.set_semiring(self.semiring_)
        own.set_mask_type(kNoMask)
        if self.row_end_ is not None:
            own.set_row_shard(self.row_begin_, self.row_end_)
        own.load_and_format_matrix(csr, True)
        own.send_matrix_host_to_device()
        self.own_pull_ = own
        self.attach_pull(own)

    def send_vector_host_to_device(self, vector):
        """The vector may be shorter than num_cols + 1; the device copy is always that long
        (spmspv_module.h:280, :379)."""
        vector = np.ascontiguousarray(vector, dtype=IDX_VAL)
        cnt = int(vector["index"][0]) if vector.shape[0] else 0
        self.hint_vector_nnz(cnt)
        self.vector_buf = capi.DeviceBuffer(8 * (self.get_num_cols() + 1))
        up = vector[:self.get_num_cols() + 1]
        if up.shape[0] and cnt + 1 > up.shape[0]:
            # the head claims more entries than the vector holds (the reference would read its zero-initialised mirror):
            # device blocks are recycled memory, so the head is clamped to what is uploaded
            up = up.copy()
            up["index"][0] = cnt = up.shape[0] - 1
        self.vector_buf.write(up)
        # the host holds the CSC: remember the vector's size, the non-zeros of its columns and the longest of them, see run()
        # (gl_spmspv_plan_hint_work: a tiny vector runs as one launch, and one below the direction switch's threshold without
        # the decision kernels)
        self.tiny_ = None
        BaseModule.device_writes_ += 1
        if 0 < cnt < vector.shape[0] and self.csc_matrix_ is not None:   # (a row shard holds no more than the whole matrix)
            cols = vector["index"][1:1 + cnt].astype(np.int64)
            cols = cols[cols < self.get_num_cols()]
            ip = self.csc_matrix_.adj_indptr
            lens = ip[cols + 1].astype(np.int64) - ip[cols].astype(np.int64)
            self.tiny_ = (cnt, int(lens.sum()), BaseModule.device_writes_, int(lens.max()) if lens.shape[0] else 0)

    def send_mask_host_to_device(self, mask):
        mask = np.ascontiguousarray(mask, dtype=np.float32)
        self.mask_buf = capi.DeviceBuffer(4 * mask.shape[0])
        self.mask_buf.write(mask)

    def bind_mask_buf(self, src_buf):
        self.mask_buf = src_buf

    def bind_vector_buf(self, src_buf):
        self.vector_buf = src_buf
        self.tiny_ = None

    def _hint_tiny(self):
        """Before a run: is the vector still the tiny one this module uploaded (no module call has written since)?"""
        t = getattr(self, "tiny_", None)
        if t is not None and t[2] == BaseModule.device_writes_:
            self.plan_.hint_work(t[0], t[1], t[3])
            return True
        self.tiny_ = None
        return False

    def run(self):
        mask = self.mask_buf if self.mask_type_ != kNoMask else None
        tiny = self._hint_tiny()
        self.plan_.run(self.vector_buf, mask, self.results_buf, self.semiring_.op, self.semiring_.zero,
                       self.mask_type_)
        self._finish_run(self.results_buf)
        if tiny:      # this run wrote the results and the accumulator, not the vector
            self.tiny_ = (self.tiny_[0], self.tiny_[1], BaseModule.device_writes_, self.tiny_[3])

    def run_assign(self, inout_buf, val):
        """Extension (gl_spmspv_run_assign): run() followed by AssignVectorSparseModule.run(val) with the results as
        its mask and `inout_buf` as its inout -- BFS's push iteration (app/bfs.h:146-148) -- in one call."""
        mask = self.mask_buf if self.mask_type_ != kNoMask else None
        self.plan_.run_assign(self.vector_buf, mask, self.results_buf, self.semiring_.op, self.semiring_.zero,
                              self.mask_type_, inout_buf, val)
        self._finish_run(self.results_buf, inout_buf)

    def _finish_run(self, *written):
        """A blocking run waits for the operator's own completion record (gl_spmspv_wait: the fold's last workgroup stores the
        result count to page-locked memory) instead of the whole stream, and remembers the count for get_results_nnz."""
        BaseModule._wrote(*written)
        self.nnz_known_ = None
        self.run_stamp_ = BaseModule.device_writes_
        if self.blocking:
            n = self.plan_.wait()
            if n is not None:
                self.nnz_known_ = (n, self.results_buf, BaseModule.device_writes_)

    def get_results_nnz(self):
        k = getattr(self, "nnz_known_", None)
        if k is not None and k[1] is self.results_buf and k[2] == BaseModule.device_writes_:
            return k[0]       # (no module call has written device memory since the run reported it)
        # the run's own completion record, if it kept one (no device -> host copy) -- trusted only while that run is the last
        # module call that wrote results_buf (SSSP's relax step, enqueued behind the run, only reads it: app/sssp.h:218-221)
        if not self.blocking and getattr(self.plan_, "wait", None) is not None and \
                getattr(self, "run_stamp_", None) is not None and getattr(self.results_buf, "last_write_", None) == self.run_stamp_:
            n = self.plan_.wait()
            if n is not None:
                return n
        return capi.sparse_nnz(self.results_buf)

    def send_vector_device_to_host(self):
        return self.vector_buf.read(IDX_VAL, self.get_num_cols() + 1)

    def send_mask_device_to_host(self):
        return self.mask_buf.read(np.float32)

    def send_results_device_to_host(self):
        return self.results_buf.read(IDX_VAL, self.get_num_rows() + 1)


class eWiseAddModule(BaseModule):
    def __init__(self):
        super().__init__()
        self.in_buf = self.out_buf = None

    def send_in_host_to_device(self, in_vec):
        self.in_buf = capi.DeviceBuffer.from_host(np.ascontiguousarray(in_vec, dtype=np.float32))

    def allocate_out_buf(self, length):
        self.out_buf = capi.DeviceBuffer(4 * length)

    def bind_in_buf(self, src_buf):
        self.in_buf = src_buf

    def bind_out_buf(self, src_buf):
        self.out_buf = src_buf

    def run(self, length, val):
        capi.ewise_add(self.in_buf, self.out_buf, length, val)
        self._finish(self.out_buf)

    def send_out_device_to_host(self):
        return self.out_buf.read(np.float32)


class AssignVectorDenseModule(BaseModule):
    def __init__(self):
        super().__init__()
        self.mask_type_ = None
        self.mask_buf = self.inout_buf = None

    def set_mask_type(self, mask_type):
        if mask_type == kNoMask:
            _fatal("Please set the mask type")  # assign_vector_dense_module.h:88-95
        self.mask_type_ = mask_type

    def send_mask_host_to_device(self, mask):
        self.mask_buf = capi.DeviceBuffer.from_host(np.ascontiguousarray(mask, dtype=np.float32))

    def send_inout_host_to_device(self, inout):
        self.inout_buf = capi.DeviceBuffer.from_host(np.ascontiguousarray(inout, dtype=np.float32))

    def bind_mask_buf(self, src_buf):
        self.mask_buf = src_buf

    def bind_inout_buf(self, src_buf):
        self.inout_buf = src_buf

    def run(self, length, val):
        if self.mask_type_ not in (kMaskWriteToZero, kMaskWriteToOne):
            _fatal("Invalid mask type")  # assign_vector_dense_module.h:242-245
        capi.assign_dense(self.mask_buf, self.inout_buf, length, val, self.mask_type_)
        self._finish(self.inout_buf)

    def send_mask_device_to_host(self):
        return self.mask_buf.read(np.float32)

    def send_inout_device_to_host(self):
        return self.inout_buf.read(np.float32)


class AssignVectorSparseModule(BaseModule):
    def __init__(self, generate_new_frontier):
        super().__init__()
        self.generate_new_frontier_ = bool(generate_new_frontier)
        self.mask_buf = self.inout_buf = self.new_frontier_buf = None

    def send_mask_host_to_device(self, mask):
        mask = np.ascontiguousarray(mask, dtype=IDX_VAL)
        self.mask_buf = capi.DeviceBuffer.from_host(mask)
        if self.generate_new_frontier_:
            # the new frontier can never be longer than the mask (assign_vector_sparse_module.h:238-253)
            self.new_frontier_buf = capi.DeviceBuffer(mask.nbytes)
            self.new_frontier_buf.write(np.zeros(mask.shape[0], dtype=IDX_VAL))

    def send_inout_host_to_device(self, inout):
        self.inout_buf = capi.DeviceBuffer.from_host(np.ascontiguousarray(inout, dtype=np.float32))

    def bind_mask_buf(self, src_buf):
        self.mask_buf = src_buf

    def bind_inout_buf(self, src_buf):
        self.inout_buf = src_buf

    def bind_new_frontier_buf(self, src_buf):
        if not self.generate_new_frontier_:
            _fatal("[ERROR]: this->generate_new_frontier_ should be true")
        self.new_frontier_buf = src_buf

    def _max_entries(self):
        cap = self.mask_buf.nbytes // 8 - 1
        if self.generate_new_frontier_:
            cap = min(cap, self.new_frontier_buf.nbytes // 8 - 1)
        return max(cap, 0)

    def run(self, val=None):
        if val is None:
            # SSSP mode (assign_vector_sparse_module.h:295-303)
            if not self.generate_new_frontier_:
                _fatal("[ERROR]: this->generate_new_frontier_ should be true")
            capi.assign_sparse_new_frontier(self.mask_buf, self.inout_buf, self.new_frontier_buf,
                                            self._max_entries())
        else:
            # BFS mode (assign_vector_sparse_module.h:278-292)
            if self.generate_new_frontier_:
                _fatal("[ERROR]: this->generate_new_frontier_ should be false")
            capi.assign_sparse(self.mask_buf, self.inout_buf, val, self._max_entries())
        self._finish(self.inout_buf, self.new_frontier_buf)

    def send_mask_device_to_host(self):
        return self.mask_buf.read(IDX_VAL)

    def send_inout_device_to_host(self):
        return self.inout_buf.read(np.float32)

    def send_new_frontier_device_to_host(self):
        if not self.generate_new_frontier_:
            _fatal("[ERROR]: this->generate_new_frontier_ should be true")
        return self.new_frontier_buf.read(IDX_VAL)
