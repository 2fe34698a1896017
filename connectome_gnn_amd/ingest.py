"""Resident datasets from connectivity matrices or ROI time series, built on the device.

Real cohorts start as one dense ``n x n`` connectivity matrix per subject (structural FA or streamline
counts, functional correlations); the reference README ("Extending to real HCP data") thresholds each to
its strongest connections, turns what is left into a COO edge list and derives a strength feature, per
subject in Python.  Here the cohort ``[S, n, n]`` sits in HBM and that step is three HIP launches
(csrc/ingest.hip) whose result is a ``RaggedPackedDataset`` -- what ``ResidentDataLoader``,
``SubjectStructureCache``, the ragged collate, captured steps and ``Trainer`` already take.

Semantics, per subject with matrix ``A`` (fp32, any sign, not necessarily symmetric):

* candidates are the ``m = n (n - 1)`` off-diagonal entries; a NaN candidate ranks as -inf; the diagonal is
  never a candidate and never an edge;
* the threshold ``t`` is exactly one of: ``keep=f`` (proportional: ``k = int(f * n * (n - 1) + 0.5)``),
  ``num_edges=k`` -- for both ``t`` is the candidate of descending rank ``k``, 0-based (the (k+1)-th
  largest), -inf when ``k >= m`` -- or ``min_weight=t`` (absolute: a float or a ``[S]`` tensor);
* ``i -> j`` is an edge iff ``i != j``, ``A[i, j] > t`` and ``A[i, j] > 0`` (both strict, as in
  ``synthetic.threshold_edges``; a NaN fails both): at most ``k`` edges, fewer when ties straddle the
  threshold, and a symmetric matrix gives a symmetric edge set;
* edges are in row-major order (``torch.nonzero`` of the mask), ``edge_weight = A[i, j]``;
* node features: the caller's ``[S, n, F]``, or by default ``[S, n, 1]`` with
  ``x[s, i, 0] = strength_i / (max_i strength_i + 1e-8)``, ``strength_i`` the sum over ``j`` of the kept
  ``A[i, j]`` (``ConnectomeGraph.degree()``); zeros for a subject without edges.

A density sweep is ``from_matrices`` called again on the same resident matrices; nothing is cached.

Graph-theoretic node features: ``node_measures(matrices, keep=..., measures=MEASURES)`` gives
``[S, n, len(measures)]`` at the same thresholds, and ``from_matrices(..., measures=...)`` /
``from_timeseries(..., measures=...)`` serve it as the dataset's ``x`` (``True`` stands for ``MEASURES``), with the
thresholds selected once.  Per subject, on the edge test above (``e_ij``): ``a_ij = A_ij`` and ``b_ij = 1`` where
``e_ij``, else 0; ``k_i = sum_j b_ij``; ``s_i = sum_j a_ij``; ``wmax = max a_ij``; ``u_ij = cbrt(a_ij / wmax)`` where
``e_ij``, else 0; and for a value map ``v``, ``T_i(v) = sum_{j,k} v_ki v_kj v_ij``.

* ``strength``: ``s_i / (max_i s_i + 1e-8)``, the same bits as the default feature;
* ``degree``: ``k_i / (n - 1)``, and 0 for ``n == 1``;
* ``mean_weight``: ``s_i / (k_i + 1e-8)``;
* ``clustering``: ``T_i(b) / (k_i (k_i - 1))`` if ``k_i >= 2``, else 0;
* ``weighted_clustering``: ``T_i(u) / (k_i (k_i - 1))`` if ``k_i >= 2``, else 0 -- Onnela's geometric-mean form on
  weights scaled by the subject's maximum.

For a symmetric kept set ``T_i(v) = diag(V^3)_i`` and the two clustering measures are ``networkx.clustering(G)`` and
``networkx.clustering(G, weight="weight")``.  For an asymmetric matrix the formula is the definition: nothing is
symmetrised or checked, and the value is not bounded by 1.  A subject without edges gives zeros; NaN entries are never
edges; a kept ``+inf`` propagates as IEEE says through the weight-valued measures, while ``degree`` and ``clustering``
do not see weights and stay exact (``T_i(b)`` is an integer below ``2^24`` on the exact fp32 matrix pipe).  The
triangle sums are two dense products per subject on the device (csrc/measures.hip); nothing cohort-sized exists
besides the output.  No atomics: two calls give the same bits, and so do two grids.

Shortest-path node measures: the names of ``PATH_MEASURES`` are taken wherever ``measures=`` is, in any
order and mix with those of ``MEASURES``; the columns follow the order given, the thresholds are selected once, and a
request without a path name launches what it launched before and gives the same bits (``measures=True`` still stands
for the five of ``MEASURES``).  Per subject, on the same edge test and with nothing symmetrised: ``d_ij`` is the number
of edges on a shortest directed path ``i -> ... -> j`` along kept edges (the out-neighbours of a row, as in the BFS of
``synthetic.small_world_stats``), infinite if there is none; ``R_i = {j != i : d_ij finite}``, ``r_i = |R_i|``;
``N_i = {j : e_ij}``, ``k_i = |N_i|``; ``d^(i)`` are the distances inside the subgraph induced on ``N_i`` (only edges
``e_jh`` with both ends in ``N_i``).

* ``nodal_efficiency``: ``(1 / (n - 1)) sum_{j in R_i} 1 / d_ij``, and 0 for ``n == 1``;
* ``closeness``: ``(r_i / (n - 1)) (r_i / sum_{j in R_i} d_ij)`` if ``r_i > 0``, else 0 (Wasserman-Faust);
* ``eccentricity``: ``max_{j in R_i} d_ij / (n - 1)``, and 0 if ``r_i == 0`` or ``n == 1``;
* ``local_efficiency``: ``(1 / (k_i (k_i - 1))) sum_{j != h in N_i} 1 / d^(i)_jh`` if ``k_i >= 2``, else 0 (unreachable
  pairs add 0).

For a symmetric kept set ``closeness`` is ``networkx.closeness_centrality(G, wf_improved=True)`` (for an asymmetric one
that of ``G.reverse()``: networkx takes incoming distances), ``local_efficiency`` is
``networkx.global_efficiency(G.subgraph(G[v]))``, and the means of ``nodal_efficiency`` and ``local_efficiency`` are
``networkx.global_efficiency(G)`` and ``networkx.local_efficiency(G)``.  A subject without edges gives zeros; NaN entries
are never edges; weights play no part beyond the edge test, so a kept ``+inf`` is an ordinary edge; all values lie in
``[0, 1]``.  Level counts, ``r_i``, ``sum d`` and the eccentricity are exact integers on the device: ``eccentricity`` is
the correctly rounded fp32 quotient, the other three are formed in fp64 from the integers and rounded to fp32 once.  One
launch (csrc/paths.hip): a workgroup keeps a subject's adjacency as a bitset in LDS and runs a BFS per node, so
``n <= PATH_MAX_NODES = 1024`` (a ``ValueError`` beyond); the cost of ``local_efficiency`` grows with the density
(``~ n k^2`` row reads per subject against ``n^2`` for the other three together).  No atomics: two calls give the same
bits, and so do two grids.  The fused GCN path takes ``in_channels <= 8``: a request of more than 8 columns trains on
the wide path.

Weighted shortest-path node measures: the names of ``WEIGHTED_PATH_MEASURES`` are accepted wherever
``measures=`` is -- in ``node_measures``, ``from_matrices`` and ``from_timeseries`` -- in any order and mix with the
other nine names.  Columns follow the order given.  Thresholds are selected once.  ``measures=True`` still stands for
the five of ``MEASURES``.  A request without a weighted name launches exactly what it launches today and gives the
same bits.  Everything is per subject, with matrix ``A``, threshold ``t`` and the existing edge test: ``e_ij`` iff
``i != j``, ``A_ij > t`` and ``A_ij > 0``.  Nothing is symmetrised.

Connection lengths:

* ``wmax = max_{e_ij} A_ij``.
* ``l_ij = wmax / A_ij`` where ``e_ij``, formed as one correctly rounded fp32 division.  Otherwise ``l_ij = +inf``.
* So every length is ``>= 1``, and the strongest edge has length exactly ``1.0``.
* Scaling a subject's matrix by a constant changes nothing.  This is the same normalisation that
  ``weighted_clustering`` uses.
* If all kept weights are equal, every length is exactly 1 and the weighted measures reduce to the binary ones.

Distances:

* ``dw_ij`` is the smallest sum of lengths along a directed path ``i -> ... -> j`` of kept edges.
* ``dw_ii = 0``.
* ``dw_ij = +inf`` when there is no path.
* ``R_i = { j != i : dw_ij finite }`` and ``r_i = |R_i|``.  This is the same set as the binary ``R_i``.

Measures:

* ``weighted_nodal_efficiency``: ``(1 / (n - 1)) sum_{j in R_i} 1 / dw_ij``.  It is 0 for ``n == 1``.
* ``weighted_closeness``: ``(r_i / (n - 1)) (r_i / sum_{j in R_i} dw_ij)`` if ``r_i > 0``, else 0 (Wasserman-Faust).
* ``weighted_eccentricity``: ``max_{j in R_i} dw_ij / (n - 1)``.  It is 0 if ``r_i == 0`` or ``n == 1``.  It may
  exceed 1.

Special cases:

* A subject without edges gives zeros.
* NaN entries are never edges.
* A subject with a kept non-finite weight gets unspecified values in these columns.  The call must still return,
  which a fixed round count guarantees.

Arithmetic:

* Distances are fp32 sums of fp32 lengths.
* The three row reductions (``sum 1/dw``, ``sum dw``, the max) are taken in fp64 in a fixed order and rounded to fp32
  once.
* No atomics.
* No work assignment depends on the grid, so every run and every grid gives the same bits.

One launch (csrc/wpaths.hip): a batched blocked Floyd-Warshall (min-plus), a workgroup per subject on a distance slab
of its own in the workspace -- one slab per workgroup of the launch, not per subject, so nothing cohort-sized exists
besides the output -- and ``n <= WEIGHTED_PATH_MAX_NODES = 1024`` (a ``ValueError`` beyond).  The cost is ``npad^3``
relaxations per subject (``npad``: ``n`` rounded up to the block, 32 nodes to ``n = 512`` and 16 beyond) whatever the
density.  ``path_lengths`` returns ``dw`` itself.

Functional cohorts start one step earlier, as one ROI time series per subject:
``correlation_matrices`` / ``from_timeseries`` take ``timeseries`` -- float32, contiguous, ``[S, T, n]``, one row
per frame, on a ROCm device -- and build the Pearson correlation matrices there (csrc/timeseries.hip).

* A *unit* is one (subject, window) pair.  Without ``window`` there is one unit per subject over all ``T``
  frames.  With ``window=L`` (``2 <= L <= T``) and ``stride=st`` (``>= 1``, default ``L``) subject ``s`` has
  ``W = (T - L) // st + 1`` units; unit ``u = s * W + w`` covers frames ``[w * st, w * st + L)``.
* Per unit, with its ``L`` frames ``x[t, i]``: ``m_i`` is the mean of column ``i`` and
  ``q_i = sum_t (x[t, i] - m_i)^2``, both accumulated in fp64 from the fp32 inputs as centred sums (blocked Welford,
  never ``E[x^2] - E[x]^2``); ``r[i, j] = sum_t z[t, i] z[t, j]`` with ``z[t, i] = (x[t, i] - m_i) / sqrt(q_i)``,
  operands centred and scaled in fp32, products exact to fp32 rounding on the fp32 matrix pipe, accumulation in
  fp32 over ``t`` ascending.  No atomics: two calls give the same bits.
* ``r[i, j]`` and ``r[j, i]`` are the same bits; off-diagonals are clamped to ``[-1, 1]``; ``r[i, i]`` is
  exactly ``1.0``.  A column with ``q_i == 0`` (a constant or masked ROI) has ``1 / sqrt(q_i)`` taken as 0: its
  whole row and column, diagonal included, are exactly ``0.0``, not NaN.
* ``absolute=True`` stores ``|r|``: anticorrelations are then kept by the strict ``> 0`` test of
  ``from_matrices``; by default they are dropped there, as any non-positive entry is.
* Non-finite inputs are not checked; they propagate as IEEE says.

A window sweep is ``from_timeseries`` called again on the same resident time series.

Partial correlation: ``partial_correlation(matrices, shrinkage=a)`` turns correlation matrices
``[U, n, n]`` into partial-correlation matrices there (csrc/partial.hip), and ``kind="partial"`` of
``correlation_matrices`` / ``from_timeseries`` does so to the signed correlations of the time series, in place.
Everything is per unit, with matrix ``R`` read from its UPPER triangle (``i <= j``) only.

* ROI ``i`` with ``R_ii == 0`` -- the zero row and column ``correlation_matrices`` writes for a constant or masked
  column -- is *excluded*: its pivot is taken as 1, so the factorisation of the others is untouched, and its row and
  column of the output, diagonal included, are exactly ``0.0``.
* ``C = (1 - a) R + a I`` over the other ROIs, ``a = shrinkage`` in ``[0, 1]``.
* ``P = C^-1``.  For ``i != j``, ``out_ij = -P_ij / sqrt(P_ii P_jj)``, clamped to ``[-1, 1]``; ``out_ii`` is exactly
  ``1.0``; ``out_ij`` and ``out_ji`` are the same bits.  ``absolute=True`` stores ``|out|`` (with ``kind="partial"``
  it applies to the partial values; the correlation underneath stays signed).
* A unit whose factorisation meets a pivot ``<= 0`` or a NaN gets an all-NaN matrix.  NaN entries are never edges, so
  ``from_matrices`` gives that unit no edges.  The round counts are fixed: the call always returns.
* ``shrinkage == 0`` needs at least ``n + 2`` frames per unit: with fewer the correlation matrix is singular by
  construction (a ``ValueError`` from ``correlation_matrices`` / ``from_timeseries``; give ``shrinkage > 0``).
* ``shrinkage`` is one float for the whole cohort, a ``[U]`` tensor with one value per unit, or, where the time series
  are at hand (``correlation_matrices`` / ``from_timeseries``), the name of an estimator from ``SHRINKAGES``.

Arithmetic: ``C = U^T U`` (blocked Cholesky, upper), ``W = U^-T``, ``P = W^T W``.  Storage and products are fp32,
every sum in ascending order, the trailing updates and ``W^T W`` on the fp32 matrix pipe.  The reciprocal pivots, the
shrunk diagonal and the scales ``1 / sqrt(P_ii)`` (``P_ii`` summed in fp64) are formed in fp64 and rounded to fp32
once.  No atomics, and no work assignment depends on the grid: every run and every grid gives the same bits.

One launch: a workgroup per unit on a slab of its own in the workspace -- one slab per workgroup of the launch, not
per unit, so nothing cohort-sized exists besides the output -- and ``n <= PARTIAL_MAX_NODES = 1024`` (a ``ValueError``
beyond: the row panel of a round must fit LDS).  About ``n^3`` multiply-adds per unit.  No solver library is called.

Shrinkage per unit, estimated from the frames: ``ledoit_wolf_shrinkage(timeseries, window=, stride=)``
gives the Ledoit-Wolf shrinkage of every unit, float64 ``[U]`` on the device, and ``shrinkage="ledoit_wolf"`` of
``correlation_matrices`` / ``from_timeseries`` with ``kind="partial"`` applies it unit by unit (what nilearn's
``ConnectivityMeasure`` does by default).  The series are standardised, so Ledoit-Wolf's target is the identity that
``partial_correlation`` shrinks towards and the estimator is two scalars per unit of ``L`` frames, with
``z[t, i] = (x[t, i] - m_i) / sqrt(q_i)`` in fp32 as the correlation kernel forms it and ``R`` the unit's matrix:

* ``p`` is the number of ROIs with ``q_i > 0`` (constant ROIs are excluded, as everywhere);
* ``s_t = sum_i z[t, i]^2`` and ``B = L sum_t s_t^2``;
* ``O = 2 sum_{i<j} R_ij^2`` and ``F = p + O``;
* ``a = 0`` if ``O == 0``, else ``(B - F) / (L O)`` clipped to ``[0, 1]``.

This is ``sklearn.covariance.ledoit_wolf_shrinkage`` of the standardised frames.  Squares, sums and the quotient are
fp64; no atomics, every merge in a fixed order: every run and every grid gives the same bits.  ``L == 2`` makes
``B - F`` zero identically and gives exactly 0; so do ``n == 1`` and a unit with one ROI that is not constant.  A
non-finite frame gives its unit a NaN.  One launch (csrc/shrinkage.hip): one read of the frames and one of the upper
triangles; ``n <= PARTIAL_MAX_NODES``.  A ``[U]`` shrinkage tensor is float64 (float32 is converted) on the matrices'
device; its values are read by the kernel only: a unit whose value is NaN or outside ``[0, 1]`` is all NaN.

Cleaning comes first: ``filter_timeseries(timeseries, t_r=, high_pass=, low_pass=)`` removes the mean,
the slow drift and what lies above the band from every column, on the device (csrc/filter.hip), and gives float32
``[S, T, n]``: what ``correlation_matrices``, ``ledoit_wolf_shrinkage`` and ``from_timeseries`` take.  It is nilearn's
``signal.clean(detrend=False, standardize=False, filter="cosine")`` extended to a low-pass, SPM's DCT drift set, an ideal
band-pass on the DCT-II grid.  Everything is per subject and per column ``i``, on the ``T`` frames of the whole run;
windows are cut afterwards.

* Basis: ``b_k[t] = sqrt(2 / T) cos(pi (2 t + 1) k / (2 T))`` for ``k = 1 .. T - 1``, the orthonormal DCT-II
  (``scipy.fft.dct(type=2, norm="ortho")``); component ``k`` has frequency ``k / (2 T t_r)`` Hz.
* Pass band, ``filter_components(T, t_r, high_pass, low_pass)``, in Python floats on the host: ``k_lo = 1`` without a
  ``high_pass``, else ``floor(2 T t_r high_pass) + 1``; ``k_hi = T - 1`` without a ``low_pass``, else
  ``min(T - 1, floor(2 T t_r low_pass))``.  The dropped low set ``1 .. k_lo - 1`` is nilearn's and SPM's cosine drift
  set for that ``high_pass``.  A band without a component is a ``ValueError``.
* Centring: ``m_i`` is the column mean, summed in fp64 in a fixed order, and ``xc[t, i] = fl32(double(x[t, i]) - m_i)``:
  one rounding.  (Subtracting an fp32 mean leaves an offset of ``2^-24 |m_i|`` that the complement form keeps.)
* Projection, with ``Kp = {k_lo .. k_hi}`` and ``Kd`` the other components: ``y = sum_{k in Kp} b_k (b_k . xc)`` if
  ``|Kp| <= |Kd|`` (the *keep* form), else ``y = xc - sum_{k in Kd} b_k (b_k . xc)`` (the *complement* form) -- the same
  function in exact arithmetic, the basis being orthonormal on the ``T`` samples; the call multiplies by the smaller
  set.  Without bounds ``y = xc`` and no product is launched.
* The smaller set holds at most ``FILTER_MAX_COMPONENTS = 256`` components (a ``ValueError`` names both counts):
  1200 frames at ``t_r = 0.72`` keep 155 in 0.01 - 0.1 Hz, and ``high_pass = 0.01`` alone drops 17.

Arithmetic: a basis value is an fp64 ``cospi`` of the exactly reduced argument ``((2 t + 1) k mod 4 T) / (2 T)``, scaled
in fp64 and rounded to fp32 once; the products run on the fp32 matrix pipe, every sum in ascending order of its index.
No atomics, and no work assignment depends on the grid: every run and every grid gives the same bits.  Columns never
mix: a constant column gives exactly ``0.0`` in every frame, and a non-finite value makes its own column of its own
subject non-finite and changes no other bit.  ``out=timeseries`` filters in place with the same bits (a workgroup owns
all frames of the columns it writes); no other overlap of ``out`` and ``timeseries`` is checked.

Confound regression: ``regress_confounds(timeseries, confounds)`` takes head motion, tissue signals and
their expansions -- ``confounds``, float32 ``[S, T, q]`` with ``1 <= q <= CONFOUND_MAX = 64``, one row per frame -- out of
every column of the time series, on the device; ``filter_timeseries(..., confounds=)`` does it after the band-pass.
Everything is per subject, in fp64 unless it says otherwise.

* Column norms: ``m_j`` is the mean of confound column ``j``, ``cc_j = c_j - m_j``, ``s_j = sqrt(sum_t cc_j[t]^2)``.  An
  exactly constant column (``s_j == 0``) is *dropped*; the others are ``u_j = cc_j / s_j``.
* Gram-Schmidt in the given column order: ``r_j = u_j - sum_{k < j, kept} q_k (q_k . u_j)`` and ``d_j = |r_j|^2``.
  Column ``j`` is *kept* iff ``d_j > CONFOUND_RANK_TOL = 1e-10``, and then ``q_j = r_j / sqrt(d_j)``; otherwise it is
  dropped: earlier columns explain it (a copy, a multiple, a sum of them).  ``rank`` is the number of kept columns.
* The basis ``Q``, ``confound_basis(confounds) -> (basis, rank)``: float32 ``[S, T, qpad]``, ``qpad`` = ``q`` rounded up
  to 32; a kept column is ``fl32(q_j)``, dropped and pad columns are exactly ``0.0``.  ``rank`` is int32 ``[S]``.
* A NaN or Inf anywhere in a subject's confounds makes its whole ``Q`` NaN and its ``rank`` -1: every output column of
  that subject is NaN, never "nothing regressed".  Other subjects keep their bits.
* Output: ``xc[t, i] = fl32(double(x[t, i]) - mean_i)`` exactly as the filter centres, and ``out = xc - Q (Q^T xc)``.

Arithmetic: the basis is a CholeskyQR2 in fp64 (csrc/confounds.hip: the Gram matrix of ``u`` summed over the frames in
ascending order by a fixed owner per pair, a ``q x q`` Cholesky in LDS whose pivot of column ``j`` is ``d_j``, the same
again with the kept set held fixed) rounded to fp32 once -- never normal equations in fp32.  The projection is
``filter_timeseries``'s kernel in complement form with one table per subject: products on the fp32 matrix pipe, sums in
ascending index order.  No atomics, and no work assignment depends on the grid: every run and every grid gives the same
bits.  Columns never mix: a constant ROI column gives exactly ``0.0``, a NaN in an ROI column stays in that column of
that subject.  ``out=timeseries`` regresses in place with the same bits.

``filter_timeseries(..., confounds=c)`` is ``regress_confounds(filter(timeseries), filter(c))`` with the same band, the
regression in place on the filter's output.  The DCT projector being orthogonal, that equals the joint regression on
``[dropped cosines | confounds]`` (Frisch-Waugh-Lovell), which is what nilearn's
``signal.clean(confounds=, filter="cosine")`` computes.  Without ``confounds`` the call launches what it always
launched and gives the same bits.

Frame censoring, or scrubbing: every time-series entry point takes ``sample_mask``, a per-subject frame
mask -- ``torch.bool`` ``[S, T]``, contiguous, on the time series' device, ``True`` = the frame is kept (what
``nilearn.interfaces.fmriprep.load_confounds(scrub=...)`` hands to ``signal.clean``).  Frames keep their place in time
and no shape changes.  A censored frame takes part in no mean, norm, inner product or count, and its stored values are
never looked at, whatever they are: selection, never multiplication.  Without ``sample_mask`` every call launches what
it always launched and gives the same bits.  For subject ``s``, ``K`` is the set of kept frames and ``Tk = |K|``.

* Centring: ``m_i`` is the mean of column ``i`` over ``K``, summed in fp64 in a fixed order;
  ``xc[t, i] = fl32(double(x[t, i]) - m_i)`` for ``t`` in ``K`` and exactly ``0.0`` elsewhere.  ``Tk == 0`` gives
  ``m_i = 0`` and zeros everywhere.
* ``confound_basis(confounds, sample_mask=)``: the statement above with every mean, norm ``s_j``, inner product and
  pivot ``d_j`` taken over ``K``.  Rows of ``Q`` at censored frames are exactly ``0.0``.  The rank rule
  (``d_j > CONFOUND_RANK_TOL``) is unchanged: once ``Tk - 1`` independent columns are kept it drops the rest, and no
  separate case handles that.  A non-finite value in a *kept* frame of a subject's confounds makes that subject's ``Q``
  NaN and its ``rank`` -1, as without a mask; one in a censored frame changes nothing.
* ``regress_confounds(timeseries, confounds, sample_mask=, out=)``: ``out = xc - Q (Q^T xc)``, products and sums as
  above.  Censored frames of ``out`` are exactly ``0.0``; on the kept frames this is the fp64 least-squares residual of
  ``x[K]`` on ``[1 | c[K]]``.
* ``filter_timeseries(..., sample_mask=)``: the cosines are not orthogonal on ``K``, so the band is removed by
  regression.  The design is one column ``fl32(b_k[t])`` for each component the band drops -- those
  ``filter_components`` leaves out, in ascending ``k``, each at the frame's own ``t`` on the grid of the whole run,
  exactly the value the filter's table holds -- followed by the confound columns if any, and
  ``out = regress_confounds(timeseries, design, sample_mask=)``: the joint residual on
  ``[1 | dropped cosines | confounds]`` sampled at the kept frames, which is what
  ``nilearn.signal.clean(filter="cosine", confounds=, sample_mask=)`` computes on the rows it returns.  Dropped
  components plus confound columns must not exceed ``CONFOUND_MAX = 64``: otherwise a ``ValueError`` names both counts
  and says that a ``low_pass`` under censoring would need the frames interpolated, which is not built; a ``low_pass``
  passes only if it fits that bound.  (That message speaks of this regression path: ``interpolate=True``, below, is the
  path that interpolates.)  With no bounds and no confounds the call is masked centring, no product launched.
* ``correlation_matrices`` / ``ledoit_wolf_shrinkage`` / ``from_timeseries(..., sample_mask=)``: a unit's frames are its
  window intersected with ``K``, ``L_u`` of them.  ``m_i`` and ``q_i`` run over those frames, as centred fp64 sums;
  ``z[t, i]`` is as above on them and ``0`` elsewhere; clamp, exact unit diagonal, mirror store, ``absolute`` and
  ``kind="partial"`` are as without a mask.  A unit with ``L_u < 2`` has ``q_i == 0`` for every ROI: by the
  constant-column rule an exactly all-zero matrix, hence a graph without edges.  Ledoit-Wolf uses ``L_u`` wherever it
  uses ``L``: ``B = L_u sum_{t kept} s_t^2``, ``a = (B - F) / (L_u O)``, and ``L_u <= 2`` or ``O == 0`` give exactly 0.
  The host-side ``ValueError`` for ``shrinkage == 0`` stays on ``L``: kept counts live on the device and are not read
  back; a unit whose kept frames make it singular is all NaN by the pivot rule.

An all-``True`` mask gives the bits of the unmasked call (``confound_basis``, ``regress_confounds``,
``correlation_matrices`` of both kinds, ``ledoit_wolf_shrinkage``).  NaN, Inf or ``1e30`` in censored frames of the series
or the confounds change no bit of any output.  An ROI that is constant over its kept frames is exactly 0, even if it
varies in censored ones; a NaN in a kept frame of an ROI stays in its column of its subject.  ``out=timeseries`` gives the
out-of-place bits.  No atomics, no read-back, and every run and every grid gives the same bits.  Deriving the mask from
framewise displacement and per-subject run lengths are not built.

Interpolating the censored frames, so that a band-pass can run under a mask:
``interpolate_censored(timeseries, sample_mask, out=)`` replaces every censored frame by a cubic spline through the
subject's kept frames, on the device (csrc/interpolate.hip), and gives float32 ``[S, T, n]``; the same call serves
confounds ``[S, T, q]``.  Per subject and per column ``i``, in fp64 unless it says otherwise: ``t_0 < .. < t_{m-1}`` are the
kept frame indices (as numbers), ``y_k = double(x[t_k, i])``, ``h_k = t_{k+1} - t_k`` and
``delta_k = (y_{k+1} - y_k) / h_k``.  ``t_r`` plays no part: the spline through the points does not change when time is
rescaled.

* Kept frames are bit copies of the input.  Whatever a censored frame holds (NaN, Inf, ``1e30``) is never looked at:
  selection, never multiplication, as above.
* ``m == 0``: every frame is exactly ``0.0``.  ``m == 1``: every frame is ``y_0``.
* Ends: a censored frame before ``t_0`` takes ``x[t_0, i]`` and one after ``t_{m-1}`` takes ``x[t_{m-1}, i]``, both as bit
  copies.  This departs from ``scipy.interpolate.CubicSpline(extrapolate=True)`` and from nilearn on purpose: a cubic
  continued over a long censored head grows without bound and would dominate the band-pass, and nilearn's alternative,
  dropping those frames, does not exist where frames keep their place.
* Inside ``(t_k, t_{k+1})``: the C2 cubic spline with not-a-knot ends (``CubicSpline``'s default) in Hermite form on the
  knot derivatives ``s_k``; with ``u = (t - t_k) / h_k``,
  ``v = (1+2u)(1-u)^2 y_k + u(1-u)^2 h_k s_k + u^2(3-2u) y_{k+1} + u^2(u-1) h_k s_{k+1}``, rounded to fp32 once.
* Knot derivatives.  ``m == 2``: ``s_0 = s_1 = delta_0`` (the line).  ``m == 3``: ``s_0 + s_1 = 2 delta_0``;
  ``h_1 s_0 + 2(h_0+h_1) s_1 + h_0 s_2 = 3(h_1 delta_0 + h_0 delta_1)``; ``s_1 + s_2 = 2 delta_1`` (the parabola through the
  three points, as scipy does).  ``m >= 4``: for ``1 <= k <= m-2``,
  ``h_k s_{k-1} + 2(h_{k-1}+h_k) s_k + h_{k-1} s_{k+1} = 3(h_k delta_{k-1} + h_{k-1} delta_k)``; first row, with
  ``d = t_2 - t_0``: ``h_1 s_0 + d s_1 = ((h_0 + 2d) h_1 delta_0 + h_0^2 delta_1) / d``; last row, with
  ``d = t_{m-1} - t_{m-3}``: ``d s_{m-2} + h_{m-3} s_{m-1} = (h_{m-2}^2 delta_{m-3} + (2d + h_{m-2}) h_{m-3} delta_{m-2}) / d``
  (scipy's rows).

Arithmetic: the system's matrix depends on the mask alone, so its Thomas factors are formed once per subject in fp64 and
a column's solve multiplies by them (no division per column); the solve, the Hermite form and the sums are fp64, one
rounding to fp32 at the store.  Columns never mix: a column constant over its kept frames gives exactly that constant in
every frame, a non-finite value in a *kept* frame stays in its column of its subject, and an all-``True`` mask gives a bit
copy.  No atomics, no read-back; every run, every grid and ``out=timeseries`` give the same bits.

``filter_timeseries(..., sample_mask=m, interpolate=True)`` is nilearn's ``signal.clean`` order for scrubbing with a
band-pass, as this sequence of public calls, bit for bit, ``o`` being the output buffer:
``o = interpolate_censored(timeseries, m, out=o)``; ``o = filter_timeseries(o, t_r=, high_pass=, low_pass=, out=o)``, the
orthogonal DCT projection centred over all ``T`` frames; then, with ``confounds=c``,
``ci = interpolate_censored(c, m)``, ``cf = filter_timeseries(ci, same band, out=ci)`` and
``o = regress_confounds(o, cf, sample_mask=m, out=o)`` -- the regression on the kept rows alone -- and without confounds
``o = filter_timeseries(o, t_r=t_r, sample_mask=m, out=o)``, masked centring.  Censored frames of the result are exactly
``0.0``, as everywhere under a mask.  The checks are the unmasked path's (a non-empty band, the smaller set at most
``FILTER_MAX_COMPONENTS``); ``interpolate=True`` without a ``sample_mask`` is a ``ValueError``.

A Butterworth band-pass instead of the cosine projection: ``filter_timeseries(..., filter="butterworth",
order=5)`` is nilearn's ``signal.clean(filter="butterworth")``, its default -- a Butterworth filter of that order run forward
and backward, zero-phase -- on the device (csrc/butterworth.hip), float32 ``[S, T, n]``; confounds ``[S, T, q]`` are served
alike.  ``filter`` is one of ``FILTERS``; with ``"cosine"``, the default, nothing above changes and ``order`` must be left
at its default.  Per subject and column ``i``, with ``sos = butterworth_sos(t_r, high_pass, low_pass, order)``:
``y = sosfiltfilt(sos, float64(x[s, :, i]))`` as ``scipy.signal.sosfiltfilt`` defines it with its defaults
(``padtype="odd"``, ``padlen=None``), and ``out[s, :, i] = fl32(y)``: one rounding.

* ``butterworth_sos`` is host code (Python floats, no scipy): the analogue prototype's poles, critical frequencies
  pre-warped, the low-pass to band or high transform, the bilinear transform, conjugate pairs into second-order sections
  ``b0 b1 b2 1 a1 a2``, float64 ``[L, 6]``.  Both bounds give a band-pass of ``order`` sections, one bound a high- or
  low-pass of ``ceil(order / 2)``; ``1 <= order <= BUTTERWORTH_MAX_ORDER = 8``.  The transfer function is
  ``scipy.signal.butter(order, ..., output="sos", fs=1 / t_r)``'s; the order of the sections and the pairing are not.
* Unlike the cosine path the result is not centred first: a low-pass keeps a column's level, as scipy and nilearn do.
* ``ValueError``s, each naming the number that decides: an ``order`` outside the range; bounds not in
  ``0 < high_pass < low_pass < 1 / (2 t_r)`` (the message names the Nyquist frequency; nilearn clips the bound and warns);
  both bounds ``None`` (the cosine filter removes the means); ``T <= edge``, scipy's pad length
  ``3 (2 L + 1 - min(#sections with b2 == 0, #sections with a2 == 0))``: 33 for the default band-pass, 18 for a 5th-order
  high- or low-pass; ``sample_mask=`` without ``interpolate=True``, a recursive filter cannot skip frames.
* ``confounds=c`` is ``regress_confounds(butter(timeseries), butter(c))``, which centres.  ``sample_mask=m,
  interpolate=True`` is the sequence above with the Butterworth call in the projection's place: the series and the
  confounds interpolated, both filtered over all ``T`` frames, the regression on the kept frames (without confounds:
  masked centring); censored frames exactly ``0.0``; bit for bit the public calls.

Arithmetic: everything is fp64.  The column is filtered as ``d = double(x) - double(x[0])`` -- the odd extension commutes
with that shift, and the initial states (``sosfilt_zi``'s, scaled by the first frame) make a constant input give a
constant output, so ``sosfiltfilt(x) = sosfiltfilt(d) + H(1)^2 x[0]`` with ``H(1)^2`` 0 for a high- or band-pass and 1 for a
low-pass, for which ``x[0]`` is added back before the one rounding.  So a constant ROI gives exactly ``0.0``, or exactly its
value under a low-pass, and an offset of 10^4 costs no accuracy.  A section is transposed direct form II,
``y = fma(b0, x, z0); z0 = fma(-a1, y, fma(b1, x, z1)); z1 = fma(-a2, y, b2 x)``; the value between the forward and the
backward pass is never rounded to fp32.  One launch, a lane per column; the forward pass keeps the states every 48 frames
only, in a workspace that depends on ``T`` and the device and not on ``S``, and the backward pass forms the forward outputs
again chunk by chunk.  A NaN anywhere in a column makes that whole column NaN and no other.  No atomics, no read-back;
every run, every grid and ``out=timeseries`` give the same bits.  The cost is the same for every band.

k-nearest-neighbour sparsification: ``keep=``, ``num_edges=`` and ``min_weight=`` compare every entry
of a subject with one number, which at the usual densities leaves weakly connected ROIs without any edge.
``knn_sparsify(matrices, k, mode="union", out=None)`` builds the other standard graph on the device (csrc/knn.hip):
every ROI keeps its ``k`` strongest connections and the picks are symmetrised.  Everything is per subject, with matrix
``A`` ``[n, n]``, fp32, any sign, not necessarily symmetric.

* Positive candidates: row ``i`` has ``P_i = { j != i : A_ij > 0 }`` and ``p_i = |P_i|``.  A NaN is not positive,
  ``+inf`` is, and the diagonal is never a candidate.
* Order: within a row ``j`` comes before ``j'`` iff ``A_ij > A_ij'``, or ``A_ij == A_ij'`` and ``j < j'``: the stable
  descending sort.
* Picks: ``D_i`` is the first ``min(k, p_i)`` members of ``P_i`` in that order, and ``d_ij`` means ``j in D_i``.  A row
  gets exactly ``min(k, p_i)`` picks; ties are broken by the lower column, and no row is left empty by a tie class that
  straddles the cut.  This is deliberately NOT the "strictly above the rank-k value" rule of ``keep=``: the guaranteed
  minimum degree is the reason the call exists.
* Modes (``KNN_MODES``): ``"directed"``: ``kept_ij = d_ij``; ``"union"``, the default and the usual k-NN graph:
  ``kept_ij = d_ij or (d_ji and A_ij > 0)``; ``"mutual"``: ``kept_ij = d_ij and d_ji``.
* Output: ``B_ij`` is the bits of ``A_ij`` where ``kept_ij`` and ``+0.0`` elsewhere; the diagonal and every NaN are
  ``+0.0`` too.

Consequences: ``from_matrices(B, min_weight=0.0)`` has exactly the edges ``kept``; a row's out-degree is at most ``p_i``
in every mode, exactly ``min(k, p_i)`` in ``"directed"`` and at least that in ``"union"``; ``mutual`` is a subset of
``directed``, which is one of ``union``; a bit-symmetric ``A`` gives a bit-symmetric ``B`` in ``"union"`` and
``"mutual"``; ``k >= n - 1`` keeps every positive off-diagonal entry (in ``"mutual"``: every one whose mirror entry
is positive too) and ``k = 0`` gives all zeros; scaling ``A`` by a
positive power of two scales ``B`` and changes no choice.  A row's picks are two numbers, the value ``v_i`` and the
column ``c_i`` of its last pick (``+inf`` and ``-1`` for a row without one):
``d_ij  <=>  A_ij > 0 and (A_ij > v_i or (A_ij == v_i and j <= c_i))``, which is what the kernel keeps per row.

One launch, ``n <= KNN_MAX_NODES = 1024`` (a ``ValueError`` beyond).  No atomics on global memory (a row's select counts
in LDS, integer adds whose order does not matter), and no work assignment depends on the
grid: every run and every grid gives the same bits, and ``out=matrices`` gives the bits of a separate output (all picks
of a subject exist before any of its entries is written).  ``knn=k`` and ``knn_mode=`` of ``from_matrices``,
``node_measures``, ``path_lengths`` and ``from_timeseries`` are a fourth way to choose the edges, refused together with
any of the other three: each call is, bit for bit, the same call on ``knn_sparsify(matrices, k, mode=knn_mode)`` with
``min_weight=0.0``.  ``from_timeseries`` sparsifies its connectivity temporary in place; the other three leave the
caller's matrices untouched and hold one cohort-sized temporary for the length of the call
(``knn_sparsify(m, k, out=m)`` and ``min_weight=0.0`` avoid it for a caller who can give the matrices up).

Maximum-spanning-tree backbone: neither a threshold nor the k-NN graph returns a connected graph; on
modular data, which connectomes are, the strongest entries all lie inside the modules.  ``mst_backbone(matrices, keep=,
num_edges=, min_weight=, out=)`` unites the choice with the maximum spanning forest of the positive weights (BCT's
``backbone_wu``; csrc/mst.hip).  Per subject with matrix ``A`` ``[n, n]``, fp32, any sign, not necessarily symmetric:

* ``p(x) = x if x > 0 else 0``: a NaN is not positive, ``+inf`` and a subnormal are.
* The pair ``{i, j}``, ``i < j``, has weight ``w_ij = max(p(A_ij), p(A_ji))`` and is a candidate iff ``w_ij > 0``.
* Order: ``(i, j)`` comes before ``(i', j')`` iff ``w > w'``, or ``w == w'`` and ``(i, j)`` is lexicographically lower:
  a strict total order, so the maximum spanning forest ``F`` (Kruskal: a pair is taken iff its ends lie in different
  components) is unique.  It has ``n - c`` pairs, ``c`` the number of components of the candidate graph; the all-0.5
  matrix gives the star at node 0.
* ``kept_ij`` iff ``i != j``, ``A_ij > 0`` and (``{i, j}`` in ``F`` or ``A_ij > t_s``), ``t_s`` the subject's threshold
  (``+inf`` without a choice: the tree alone).  A tree pair whose reverse entry is not positive keeps only the positive
  direction, as ``"union"`` does.
* Output: the bits of ``A_ij`` where kept, ``+0.0`` elsewhere, the diagonal and every NaN too.

One launch, ``n <= MST_MAX_NODES = 1024``: the symmetrised weights go to a slab per workgroup of a workspace, Prim with
restarts runs on 64-bit integer keys in registers (no subnormal is flushed), and every decision of a subject exists
before any entry is written: no atomics, the same bits on every run and grid, in place and out of place.
``backbone="mst"`` (one of ``BACKBONES``) of ``from_matrices``, ``node_measures``, ``module_profile``, ``path_lengths``
and ``from_timeseries``, together with one of the three thresholds, is bit for bit the same call on
``mst_backbone(m, <that choice>)`` with ``min_weight=0.0``; alone it is the tree alone; together with ``knn=`` it is the
same call on ``torch.maximum(knn_sparsify(m, k, mode=knn_mode), mst_backbone(m))``, which is exact because every entry is
a positive value's bits or ``+0.0``, and which holds two cohort-sized temporaries for the length of the call, the k-NN
graph and the tree (``from_timeseries``: the tree only).  The united graph has at most ``2 (n - 1)`` more entries than the
choice alone.

Module measures: the atlases ship with a partition of their ROIs into functional networks, and
``MODULE_MEASURES`` are the node descriptors built on it.  ``modules=`` of ``node_measures``, ``from_matrices`` and
``from_timeseries`` is that partition: ``n`` labels ``c_j`` in ``0 .. M - 1``, each used, ``M <= MODULE_MAX = 64``, one
per cohort, checked on the host (a sequence, an array or a CPU tensor; a device tensor is refused, since the check
would read it back).  It is given exactly when a module measure is named.  With ``e_ij``, ``a_ij``, ``b_ij`` as above
(rows are what is summed, nothing is symmetrised): ``k_i(m) = sum_{j: c_j = m} b_ij``, ``s_i(m) = sum_{j: c_j = m}
a_ij``, ``k_i = sum_m k_i(m)``, ``s_i = sum_m s_i(m)``, ``kappa_i = k_i(c_i)``, ``sigma_i = s_i(c_i)``.

* ``participation``: ``1 - sum_m (k_i(m) / k_i)^2``, 0 if ``k_i == 0``
* ``weighted_participation``: ``1 - sum_m (s_i(m) / s_i)^2``, 0 if ``s_i == 0``
* ``module_zscore``: ``(kappa_i - mean) / std`` over the nodes of module ``c_i`` (population std, as numpy and BCT);
  0 if all ``kappa`` of that module compare equal (that test, not ``std == 0``: BCT sets those NaNs to 0)
* ``weighted_module_zscore``: the same on ``sigma_i``
* ``diversity``: ``-sum_{m: p > 0} p ln p / ln M`` with ``p = s_i(m) / s_i``; 0 if ``s_i == 0`` or ``M == 1``

Everything after the fp32 edge test is fp64 in a fixed order, rounded to fp32 once; the binary sums are exact integers.
A kept ``+inf`` follows the formulas: NaN in that row's weighted columns and in the weighted z-scores of its module.
One launch (csrc/modules.hip), a wave per row with the row in registers (``n <= MODULE_MAX_NODES = 1024``), the
z-scores in a second phase over LDS that runs only when one is asked for; no workspace, no atomics, no read-back, the
same bits on every run and for every grid.  ``module_profile(matrices, modules, binary=False, normalize=False)``
returns the network profile ``s_i(m)`` (``k_i(m)`` if ``binary``; divided by the row total if ``normalize``, an
isolated node keeping an exact zero row) as ``[S, n, M]``: with the 7 Yeo networks that is 7 feature columns, which as
``node_features=`` keep a cohort on the fused GCN path (``in_channels <= 8``).

Series features: everything above describes the thresholded matrix, which message passing sees anyway;
``series_features(timeseries, t_r=, band=, features=SERIES_FEATURES)`` describes the series themselves, how strongly and
how slowly each region fluctuates, as ``[S, n, F]``, which ``node_features=`` takes.  Per subject and column, stated in
fp64 on the fp32 input: ``xc = x - mean``, ``q = sum xc^2``, ``X_k = sum_t xc[t] exp(-2 pi i k t / T)`` for
``k = 1 .. K = T // 2`` (``numpy.fft.rfft``), ``w_k = 2`` but ``w_K = 1`` for even ``T``, and the band is the bins
``series_band(T, t_r, band)``: ``k_lo = max(1, ceil(lo T t_r))`` to ``k_hi = min(K, floor(hi T t_r))``.

* ``std``: ``sqrt(q / (T - 1))``, BOLD variability
* ``autocorr1``: ``sum_{t < T-1} xc[t] xc[t+1] / q``
* ``alff``: the mean over the band of ``2 |X_k| / T`` (Zang 2007; REST and DPABI without their zero-padding)
* ``falff``: ``sum_band |X_k| / sum_{k = 1 .. K} |X_k|`` (Zou 2008)
* ``band_std``: ``sqrt(sum_band w_k |X_k|^2 / T / (T - 1))``, the sample std of the ideally band-passed column: C-PAC's ALFF
* ``band_fraction``: ``band_std / std``: C-PAC's fALFF

A zero denominator gives ``+0.0``, so a constant column is exactly ``+0.0`` in every feature; a NaN makes the features of
its own column NaN and no other.  The mean, ``q`` and the lag-1 sum are fp64 on the unrounded ``xc``; the spectrum is a
product with a cos/sin table of the bins asked for on the fp32 matrix pipe (csrc/activity.hip), ``|X_k|^2``, its root, the
sums, ratios and roots in fp64, one rounding; no coefficient is stored.  ``falff`` alone walks the whole spectrum: its table
is ``[T, 2 K]`` floats, hence ``T <= SERIES_MAX_FRAMES`` for the spectral names, and it costs ``K / (k_hi - k_lo + 1)``
times the band's product; ``band_fraction`` is the cheap substitute.

Centrality: ``centrality_measures(matrices, keep=.., measures=CENTRALITY_MEASURES, damping=0.85)`` gives
the PageRank of every node, the one measure here of the recursive kind (a node matters because its neighbours do), as
``[S, n, len(measures)]``, which ``node_features=`` takes.  With the edge test ``e_ij`` above, entry ``(i, j)`` an edge
``j -> i``, ``w_ij = A_ij`` (``weighted_pagerank``) or 1 (``pagerank``) where ``e_ij``, and ``c_j = sum_i w_ij`` the
out-strength of ``j`` (a column sum: the row sum on the symmetric matrices of real cohorts), ``x`` is the solution of
``x_i = d (sum_j w_ij x_j / c_j + (sum_{c_j == 0} x_j) / n) + (1 - d) / n``, which sums to 1: a dangling node's mass is
spread uniformly (networkx's convention).  The solution is unique on any graph, disconnected ones included.  Everything
after the fp32 edge test is fp64, rounded to fp32 once: the iteration from ``x = 1 / n``, two products a step, stops at
the first step whose L1 change is at most ``(1 - d) 2^-42``, which leaves ``2^-42`` in L1, at the latest after
``ceil(43 ln 2 / -ln d) + 2`` steps (186 at ``d = 0.85``; never reached in exact arithmetic).  A subject without kept
entries is exactly ``1 / n``; a kept ``+inf`` makes that subject's ``weighted_pagerank`` NaN and nothing else.  One launch (csrc/pagerank.hip), a workgroup per subject with its kept entries
compacted into LDS where they fit (``n <= PAGERANK_MAX_NODES = 1024``); no workspace, no atomics, no read-back, the same
bits on every run, for every grid and for every subset and order of the two names.

Cores: ``core_measures(matrices, keep=.., measures=CORE_MEASURES)`` answers not "how many neighbours"
but "how deep inside the densely connected core": a leaf on a hub and a member of a 20-clique can share a degree and
differ widely here.  With ``e_ij``, ``a_ij`` and ``b_ij`` as above, ``k_i(H) = sum_{j in H} b_ij`` and
``s_i(H) = sum_{j in H} a_ij`` for a node set ``H`` (rows are what is summed; nothing is symmetrised), the generalised
core value of Batagelj & Zaversnik for ``p = k`` or ``p = s`` is ``c(i) = max_{H containing i} min_{u in H} p_u(H)``,
unique on any graph.  It is computed by peeling in rounds: ``L = 0``, ``r = 0``, all nodes alive; while a node is alive,
``r += 1``, ``L = max(L, min over alive u of p_u(alive))`` and every alive ``u`` with ``p_u(alive) <= L`` is removed
together, with value ``L`` and layer ``r``.

* ``coreness``: ``k_i / (n - 1)`` with ``k_i`` the value for ``p = k``, the k-core number (``networkx.core_number`` on a
  symmetric kept set; BCT's ``kcoreness_centrality_bu``); 0 for ``n == 1``; at most ``degree``
* ``onion_layer``: ``r_i / n`` with ``r_i`` the layer for ``p = k`` (``networkx.onion_layers``; an isolated node is in
  layer 1 of core 0)
* ``s_coreness``: ``sigma_i / (max_i s_i(all) + 1e-8)`` with ``sigma_i`` the value for ``p = s``, the s-core level of
  BCT's ``score_wu``, over ``strength``'s normaliser; at most ``strength``

``k_i`` and ``r_i`` are exact integers and the first two columns one correctly rounded fp32 quotient.  Everything of
``s`` after the edge test is fp64, rounded to fp32 once, and every ``s_u(alive)`` is summed anew from 0.0 over the row's
kept entries at alive columns in ascending column order -- a removed neighbour is left out, never subtracted from a
running sum -- so the rounded ``s`` is still monotone and the peeling is exactly its generalised core.  A kept ``+inf``
makes that subject's ``s_coreness`` NaN and nothing else.  ``core_levels`` gives ``k_i``, ``r_i`` and the weighted layer
``rho_i`` as int32 ``[S, n, 3]``.  One launch (csrc/core.hip), a workgroup per subject with its adjacency bitset in LDS
(``n <= CORE_MAX_NODES = 1024``) and, where they fit, its kept weights beside it; no workspace, no atomics, no read-back,
the same bits on every run, for every grid and for every subset and order of the three names.

Random-walk encodings: ``random_walk_encodings(matrices, keep=.., steps=8)`` is the structural
encoding a GNN user reaches for first (RWSE: Dwivedi et al. 2022, PyG's ``AddRandomWalkPE``): the probability that a
``k``-step random walk from a node is back at it.  With ``e_ij`` as above, ``a_ij = A_ij`` on edges (``1`` on edges with
``binary=True``) and ``0`` elsewhere, ``s_i = sum_j a_ij`` and ``P_ij = a_ij / s_i`` (an exact zero row where
``s_i == 0``; rows are what is summed, nothing is symmetrised), the column of step ``k`` is ``r_k(i) = ((P)^k)_ii``.
That is the definition for asymmetric input too; on a symmetric kept set it is ``AddRandomWalkPE``.  Every value lies in
``[0, 1]`` and is unique on the disconnected graphs a threshold returns.  ``r_1``, an isolated node's row, a subject
without edges and ``n == 1`` are exactly ``0.0``, and so is every odd step on a bipartite kept set; a kept ``+inf``
(weights only: ``binary=True`` never reads a weight as a number) makes that subject's columns for ``k >= 2`` NaN and
nothing else.  Arithmetic: ``s_i`` is an fp64 sum in ascending column order rounded to fp32 once, ``P_ij`` one fp32
division, ``M2 = P P``, ``M3 = P M2`` and ``M4 = M2 M2`` are fp32 products on the matrix pipe with ``k`` ascending (only
those the largest step needs), and ``r_k(i) = sum_j (M_a)_ij (M_b)_ji`` with ``a = k // 2``, ``b = k - a`` and
``M1 = P`` is an fp64 sum of exact products in ascending ``j``, rounded to fp32 once:
``|r_k - fp64| <= 1.01 ((k - 2) n + 2 k + 1) 2^-24 |r_k| + 2^-40``.  One launch (csrc/rw.hip), persistent workgroups
with a grid stride over the subjects, the intermediates in a slab set per workgroup (``n <= RW_MAX_NODES = 1024``;
``P`` is never stored); no cohort-sized temporary, no atomics, no read-back, the same bits on every run, for every grid
and for every subset and order of the steps.

Group-consensus edges: every choice above is made inside one subject's matrix, so every subject gets a
graph of its own and the differences are mostly noise.  ``group=`` of ``from_matrices``, ``node_measures``,
``module_profile``, ``path_lengths``, ``centrality_measures``, ``core_measures``, ``random_walk_encodings`` and
``from_timeseries`` changes whose matrix the choice is
made on: the whole edge choice (one of the three thresholds; or ``knn=`` / ``knn_mode=``; with or without
``backbone="mst"``) is applied to a group matrix ``G`` ``[n, n]`` as a cohort of one unit, and every subject is masked to
that edge set.  ``group_matrix(matrices, statistic, among=)`` gives ``G`` (csrc/group.hip), ``statistic`` one of
``GROUP_STATISTICS``; ``N`` is the number of included units, those with ``among[s]`` true (all, without ``among``).

* The sum, per entry ``(i, j)``, in fp64, in an order that depends on neither the grid nor the run: the units are cut
  into slices of 64 consecutive units (``CGNN_GROUP_SLICE``); a slice's partial starts at ``0.0`` and adds its included
  units in ascending order; the partials are folded in ascending slice order from ``0.0``.
* ``"mean"``: ``sum_s A_sij / N``.  ``"fisher_mean"``: ``tanh(sum_s atanh(A_sij) / N)``, fp64 ``atanh`` and ``tanh``.
  ``"consistency"`` (van den Heuvel & Sporns): ``count_s[i != j and A_sij > t_s and A_sij > 0] / N``, the edge test above
  at every unit's own threshold ``t_s`` -- exactly one of ``keep=`` / ``num_edges=`` / ``min_weight=`` (``[S]`` as a
  tensor), which the other two statistics refuse; the count is an exact integer.
* One fp64 division and one rounding to fp32, and no special case: ``N == 0`` gives NaN everywhere; a NaN in an included
  unit makes that entry NaN; ``+inf`` and ``-inf`` in the same entry give NaN; ``|r| == 1`` goes through ``atanh`` as
  ``+-inf``; the diagonal is reduced like any entry, except that ``"consistency"`` leaves it at 0; a bit-symmetric cohort
  gives a bit-symmetric ``G``.
* A unit left out by ``among`` is never read: NaN, Inf or ``1e30`` there change no bit (the rule ``sample_mask=`` follows
  for frames), and an all-True ``among`` gives the bits of the call without it.
* The group edge set: ``(G', t) = `` the edge choice applied to ``G[None]``; ``E = {(i, j): i != j, G'_ij > t and
  G'_ij > 0}``; a NaN group entry is never an edge.
* The mask, ``group_sparsify(matrices, group, <the choice>, out=)``: ``out_sij`` is the bits of ``A_sij`` if ``(i, j)`` is
  in ``E`` and ``A_sij > 0``, else ``+0.0`` (the diagonal, every NaN and ``-0.0`` too); ``out=matrices`` gives the same
  bits.  ``group`` is ``"mean"``, ``"fisher_mean"`` or a float32 ``[n, n]`` tensor on the device; ``"consistency"`` as a
  string is refused, it needs a threshold choice of its own.

Each call with ``group=`` is, bit for bit, the same call on ``group_sparsify(matrices, group, <the choice>)`` with
``min_weight=0.0``; the caller's matrices are left alone and the masked cohort is the one cohort-sized temporary
(``from_timeseries`` masks its connectivity temporary in place; its units are the windows).  A subject whose entry at a
group edge is not positive drops that edge, so subjects' edge sets are subsets of ``E``.  The statistic streams the cohort
once into a workspace ``1 / 32`` its size and folds it (two launches), the mask copies it once (one launch); no atomics, no
read-back, the same bits on every run and for every grid.  Without ``group=`` every call launches what it launched before.

Rank correlation: Pearson and partial correlation are moment estimators, so a few spiky frames decide an
edge; scrubbing helps only where the bad frames are known.  Spearman's rho needs no frame list, and it is the Pearson
correlation of the mid-ranks, so the one new step is the ranking: ``rank_timeseries(timeseries, window=, stride=,
sample_mask=)`` gives float32 ``[U, L, n]`` (``[S, T, n]`` without a window), per unit and column over the unit's kept
frames ``rank(t) = 1 + #{t': v_t' < v_t} + (#{t': v_t' == v_t} - 1) / 2``, ``scipy.stats.rankdata(method="average")``.
The comparisons are the IEEE ones of the fp32 values, on order-preserving integer keys: ``-0.0 == +0.0``, ``+-inf`` are
ordinary values, subnormals are distinct and never flushed.  A NaN in a kept frame makes the kept frames of that column
of that unit NaN and nothing else; a censored frame is exactly ``0.0`` and its value is never looked at; a column that is
constant on its ``L_u`` kept frames is ``(L_u + 1) / 2`` there, which the correlation's constant-ROI rule turns into an
exact zero row and column.  Every value is a multiple of ``1/2`` up to ``RANK_MAX_FRAMES = 4096``, exact in fp32: the
output is the fp32 cast of the statement bit for bit, on every run, for every grid, and in place (``out=timeseries``,
without a window).  ``rank=True`` of ``correlation_matrices``, ``from_timeseries`` and ``ledoit_wolf_shrinkage`` is, bit
for bit, the same call without a window on ``rank_timeseries(timeseries, window=, stride=, sample_mask=)`` with the mask
unfolded to ``[U, L]``; ranking is an argument beside ``kind``, not a kind, so ``rank=True, kind="partial"`` is the
partial Spearman correlation.  The ranked series is one temporary ``[U, L, n]``: the size of the input without a window,
``W L / T`` times it with one; it is freed before the call returns.  One launch (csrc/rank.hip): persistent workgroups
over (unit, 4 adjacent columns), the columns staged in LDS as (key, frame) pairs, a wave sorting a column (bitonic), tie
runs by neighbour comparison and two scans; no workspace, no atomics, no read-back.  Left out: rank-based inverse-normal
scores, units of more than 4096 frames.

Kendall's tau: the other rank estimator, concordant minus discordant pairs of frames, with a proper
treatment of ties.  Over the pairs ``k = (s < t)`` of a unit's kept frames and ``a_ik = sign(x_si - x_ti)``, ``G = A^T A``
is an integer Gram matrix: ``G_ij`` is concordant minus discordant, ``G_ii = L_u (L_u - 1) / 2 - n1_i`` the pairs not tied
in column ``i``, and ``tau_b(i, j) = G_ij / sqrt(G_ii G_jj)``: the tie correction is the diagonal of the same product.
``kendall_counts(timeseries, window=, stride=, sample_mask=)`` gives ``G``, int32 ``[U, n, n]``, exact and bit-symmetric;
``kendall_matrices(..., absolute=)`` gives tau-b, float32, ``fp32(G_ij / sqrt(G_ii G_jj))`` formed in fp64 and rounded
once: ``scipy.stats.kendalltau``.  The diagonal is exactly 1; a column that is constant over its kept frames
(``G_ii == 0``) is an exact zero row and column, diagonal included -- the correlation's constant-ROI rule, where scipy
gives NaN; a column with a NaN in a kept frame has ``G_ii = -1`` and zeros elsewhere in its row and column, NaN in the
matrices, and touches nothing else; a unit with fewer than two kept frames is all zeros; a censored frame takes part in
no pair and is never looked at; ``|tau| <= 1``.  The comparisons are the ranking's: the calls rank first (the path
``rank=True`` takes, the ranked series ``[U, L, n]`` being the one temporary) and the kernel compares 16-bit keys, twice
the mid-ranks, so ``L <= KENDALL_MAX_FRAMES = 4096``.  ``kendall=True`` of ``correlation_matrices`` and
``from_timeseries`` is an argument beside ``rank`` and ``kind``, not a kind: bit for bit ``kendall_matrices``, with
``kind="partial"`` and a float or ``[U]`` shrinkage ``partial_correlation`` of the signed tau matrices written over them
(a normalised Gram matrix is positive semidefinite), handed to every edge choice and to ``measures=`` unchanged.  It is
refused with ``rank=True`` (tau is a function of the ranks alone) and with ``shrinkage="ledoit_wolf"`` (a statement about
the frames of a Pearson matrix).  Launches (csrc/kendall.hip): the ranking; the counts, persistent workgroups over (unit,
pair of 96-column tiles) that form the sign bytes of 64-frame block pairs once in LDS and multiply them on the int8 matrix
pipe (``v_mfma_i32_16x16x64_i8``, int32 sums: the same bits on every run and for every grid, no atomics); and the
normalisation, which without a request for the counts runs in place over them.  Left out: tau-a and tau-c, p-values,
units of more than 4096 frames.
"""
from __future__ import annotations

import ctypes
import cmath
import itertools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .synthetic import RaggedPackedDataset

_LIMIT = 2 ** 31
MEASURES = ("strength", "degree", "mean_weight", "clustering", "weighted_clustering")   # ids: include/cgnn.h
PATH_MEASURES = ("nodal_efficiency", "closeness", "eccentricity", "local_efficiency")      # ids: include/cgnn.h
PATH_MAX_NODES = 1024                                 # CGNN_PATH_MAX_NODES: the adjacency bitset must fit LDS
WEIGHTED_PATH_MEASURES = ("weighted_nodal_efficiency", "weighted_closeness", "weighted_eccentricity")   # ids: cgnn.h
WEIGHTED_PATH_MAX_NODES = 1024                        # CGNN_WPATH_MAX_NODES: both panels of a round must fit LDS
PARTIAL_MAX_NODES = 1024                              # CGNN_PARTIAL_MAX_NODES: the row panel of a round must fit LDS
KINDS = ("correlation", "partial")                    # correlation_matrices's kind=
SHRINKAGES = ("ledoit_wolf",)                         # correlation_matrices's shrinkage=, besides a float or a tensor
FILTER_MAX_COMPONENTS = 256                           # CGNN_FILTER_MAX_COMPONENTS: the coefficients of 64 columns must fit LDS
_FILTER_MAX_FRAMES = 2 ** 30                          # cgnn_ingest_filter's bound on T
CONFOUND_MAX = 64                                     # CGNN_CONFOUND_MAX: the widest table of k_filter's regress form
CONFOUND_RANK_TOL = 1e-10                             # CGNN_CONFOUND_RANK_TOL: a column is kept iff its pivot d_j exceeds it
FILTERS = ("cosine", "butterworth")                   # filter_timeseries's filter=
BUTTERWORTH_MAX_ORDER = 8                             # CGNN_BUTTER_MAX_SECTIONS (cgnn_butterworth.h): a band-pass has `order` sections
_BUTTERWORTH_ORDER = 5                                # nilearn's
KNN_MODES = ("union", "mutual", "directed")           # knn_sparsify's mode=, knn_mode= elsewhere
KNN_MAX_NODES = 1024                                  # CGNN_KNN_MAX_NODES (cgnn_knn.h): a row lives in 16 registers per lane
_KNN_MODE_IDS = {"union": _lib.KNN_UNION, "mutual": _lib.KNN_MUTUAL, "directed": _lib.KNN_DIRECTED}
BACKBONES = ("mst",)                                  # backbone= of the matrix entry points
MST_MAX_NODES = 1024                                  # CGNN_MST_MAX_NODES (cgnn_mst.h): a lane owns 4 nodes of the tree phase
MODULE_MEASURES = ("participation", "weighted_participation", "module_zscore", "weighted_module_zscore",
                   "diversity")                       # ids: include/cgnn_modules.h
MODULE_MAX = 64                                       # CGNN_MODULE_MAX: a lane of a wave owns a module
MODULE_MAX_NODES = 1024                               # CGNN_MODULE_MAX_NODES: a row lives in 16 registers per lane
SERIES_FEATURES = ("std", "autocorr1", "alff", "falff", "band_std", "band_fraction")   # ids: include/cgnn_activity.h
SERIES_MAX_FRAMES = 4096                              # CGNN_ACTIVITY_MAX_FRAMES: falff's table [T, 2 (T // 2)] stays <= 64 MB
_SERIES_SPECTRAL = SERIES_FEATURES[2:]                # the names that need t_r and a band
CENTRALITY_MEASURES = ("pagerank", "weighted_pagerank")   # ids: include/cgnn_pagerank.h
PAGERANK_MAX_NODES = 1024                             # CGNN_PAGERANK_MAX_NODES: a kept entry's column is stored in 16 bits
PAGERANK_MAX_DAMPING = _lib.PAGERANK_MAX_DAMPING      # CGNN_PAGERANK_MAX_DAMPING: the step bound grows as 1 / (1 - d)
GROUP_STATISTICS = ("mean", "fisher_mean", "consistency")   # ids: include/cgnn_group.h
CORE_MEASURES = ("coreness", "onion_layer", "s_coreness")   # ids: include/cgnn_core.h
CORE_MAX_NODES = 1024                                 # CGNN_CORE_MAX_NODES: the adjacency bitset must fit LDS
RW_MAX_STEPS = 8                                      # CGNN_RW_MAX_STEPS: M2, M3 and M4 reach step 8
RW_MAX_NODES = 1024                                   # CGNN_RW_MAX_NODES: the fp32 row sums of a subject live in LDS
RANK_MAX_FRAMES = 4096                                # CGNN_RANK_MAX_FRAMES: a unit's (key, frame) pairs of 4 columns must fit LDS
KENDALL_MAX_FRAMES = 4096                             # CGNN_KENDALL_MAX_FRAMES: keys 2 x mid-rank <= 8192 in 16 bits, counts < 2^23


class _Family(NamedTuple):
    """One C entry point and the measures it writes; a measure's id is its position in ``names``."""
    names: tuple
    call: str                                         # the byte-count query is call + "_workspace_bytes"
    cols: bool                                        # takes cols / ldx: writes its columns inside a wider x
    dist: bool                                        # takes dist / dist_bytes
    max_nodes: Optional[int] = None                   # the largest n, and for the message who is limited and why
    what: str = ""
    why: str = ""
    modules: bool = False                             # takes modules / M, and profile / profile_bytes / profile_flags
    tail: tuple = ()                                  # what follows x / x_bytes when no more than x is asked for


_FAMILIES = (                                         # in the order of their calls
    _Family(MEASURES, "cgnn_ingest_measures", False, False),
    _Family(PATH_MEASURES, "cgnn_ingest_paths", True, False, PATH_MAX_NODES, "path measures",
            "the adjacency bitset of a subject must fit LDS"),
    _Family(WEIGHTED_PATH_MEASURES, "cgnn_ingest_wpaths", True, True, WEIGHTED_PATH_MAX_NODES,
            "weighted path measures", "both panels of a Floyd-Warshall round must fit LDS", tail=_lib.buf(None)),
    _Family(MODULE_MEASURES, "cgnn_ingest_modules", True, False, MODULE_MAX_NODES, "module measures",
            "a row lives in 16 registers per lane", modules=True, tail=_lib.buf(None) + (0,)))
_WEIGHTED = _FAMILIES[2]                              # path_lengths's
_MODULES = _FAMILIES[3]                               # module_profile's
_ALL_MEASURES = tuple(name for fam in _FAMILIES for name in fam.names)
# centrality_measures's: a call of its own, so not among _FAMILIES, whose names measures= takes (damping stands in front
# of the workspace, iterations / iterations_bytes follow x)
_CENTRALITY = _Family(CENTRALITY_MEASURES, "cgnn_ingest_pagerank", True, False, PAGERANK_MAX_NODES,
                      "centrality measures", "a kept entry's column is stored in 16 bits", tail=_lib.buf(None))
# core_measures's and core_levels's: likewise a call of its own (levels / levels_bytes follow x)
_CORE = _Family(CORE_MEASURES, "cgnn_ingest_cores", True, False, CORE_MAX_NODES, "core measures",
                "the adjacency bitset of a subject must fit LDS", tail=_lib.buf(None))
# random_walk_encodings's: likewise a call of its own; the "names" are the steps 1 .. RW_MAX_STEPS, step k has id k - 1
# (the flags stand in front of the workspace)
_RW = _Family(tuple(range(1, RW_MAX_STEPS + 1)), "cgnn_ingest_rw", True, False, RW_MAX_NODES, "random-walk encodings",
              "the fp32 row sums of a subject live in LDS")


def _check_matrices(matrices) -> tuple:
    if not isinstance(matrices, torch.Tensor):
        raise TypeError(f"matrices must be a torch.Tensor, got {type(matrices).__name__}")
    if matrices.dtype != torch.float32:
        raise TypeError(f"matrices must be float32, got {matrices.dtype}")
    if matrices.dim() != 3 or matrices.shape[1] != matrices.shape[2] or matrices.shape[1] == 0:
        raise ValueError(f"matrices must be [S, n, n] with n >= 1, got {tuple(matrices.shape)}")
    S, n = int(matrices.shape[0]), int(matrices.shape[1])
    if S * n >= _LIMIT:
        raise ValueError(f"S * n = {S * n} >= 2^31: ingest the cohort in slices of subjects")
    if n * n >= _LIMIT:
        raise ValueError(f"n * n = {n * n} >= 2^31: matrices this large are not supported")
    return S, n


def _rank(n: int, keep, num_edges) -> int:
    if (keep is None) == (num_edges is None):
        raise ValueError("give exactly one of keep= and num_edges=")
    if keep is not None:
        keep = float(keep)
        if not 0.0 <= keep <= 1.0:                    # (a NaN is refused here too)
            raise ValueError(f"keep must lie in [0, 1], got {keep}")
        return int(keep * n * (n - 1) + 0.5)
    if isinstance(num_edges, bool) or not isinstance(num_edges, int):
        raise TypeError(f"num_edges must be an int, got {type(num_edges).__name__}")
    if num_edges < 0:
        raise ValueError(f"num_edges must be >= 0, got {num_edges}")
    return min(num_edges, _LIMIT)                     # anything >= n (n - 1) keeps every positive entry


def _threshold_choice(n: int, units: int, unit_name: str, keep, num_edges, min_weight) -> tuple:
    """``(k, min_weight)`` of a valid choice, exactly one of the three: the rank ``k`` of ``keep=`` / ``num_edges=``
    (``min_weight`` None), or ``k = 0`` and ``min_weight`` as a float or as the ``[units]`` tensor it is."""
    if sum(a is not None for a in (keep, num_edges, min_weight)) != 1:
        raise ValueError("give exactly one of keep=, num_edges= and min_weight=")
    if min_weight is None:
        return _rank(n, keep, num_edges), None
    if not isinstance(min_weight, torch.Tensor):
        return 0, float(min_weight)
    if min_weight.shape != (units,) or not min_weight.is_floating_point():
        raise ValueError(f"a min_weight tensor must be floating point [{unit_name}] = [{units}], got "
                         f"{min_weight.dtype} {tuple(min_weight.shape)}")
    return 0, min_weight


_MATRICES = ("matrices", "thresholds connectivity matrices")         # _require_resident's noun and verb phrase
_SERIES = ("timeseries", "correlates ROI time series")
_CONFOUNDS = ("confounds", "orthonormalises confounds")


def _require_resident(data: torch.Tensor, noun: str, does: str) -> None:
    if not data.is_contiguous():
        raise ValueError(f"{noun} must be contiguous")
    if not data.is_cuda:
        raise RuntimeError(
            f"{noun} are on {data.device}: connectome_gnn_amd {does} on a ROCm "
            "device only (there is no CPU fallback; move them with .to('cuda')).")


_WORK = object()                                      # among _call's arguments: where the workspace goes


def _call(dev, name: str, *args, workspace=None) -> None:
    """``_lib.call(name, *args)`` on ``dev``.  ``workspace=(call, *arguments)``: ``call + "_workspace_bytes"`` is asked
    first (its answer may depend on the device's grid), a negative answer is refused, and ``_WORK`` among ``args``
    becomes the pointer and the byte count of a uint8 buffer of that size (no buffer for 0 bytes)."""
    with _lib.device_guard(dev):
        if workspace is not None:
            query = workspace[0] + "_workspace_bytes"
            need = getattr(_lib.load(), query)(*workspace[1:])
            if need < 0:                              # (the message names the sizes: the integers in front)
                sizes = itertools.takewhile(lambda a: isinstance(a, int), workspace[1:])
                raise _lib.CgnnError(f"{query}({', '.join(map(str, sizes))}) refused its arguments")
            at = next(i for i, a in enumerate(args) if a is _WORK)     # (by identity: tensors define ==)
            work = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
            args = args[:at] + _lib.buf(work) + args[at + 1:]
        _lib.call(name, *args, device=dev)


def _thresholds(matrices: torch.Tensor, k: int, min_weight) -> torch.Tensor:
    """The ``[S]`` float32 thresholds of ``_threshold_choice``'s pair on the resident matrices' device: the entries of
    rank ``k``, selected there (cgnn_ingest_select), or ``min_weight``."""
    S, n = int(matrices.shape[0]), int(matrices.shape[1])
    if min_weight is None:
        thr = torch.empty(S, dtype=torch.float32, device=matrices.device)
        _call(matrices.device, "cgnn_ingest_select", matrices, S, n, k, *_lib.buf(thr))
        return thr
    if isinstance(min_weight, torch.Tensor):
        return min_weight.to(device=matrices.device, dtype=torch.float32).contiguous()
    return torch.full((S,), min_weight, dtype=torch.float32, device=matrices.device)


class _Series(NamedTuple):
    """A valid request: S subjects of T frames and n ROIs; L frames per unit, st frames between units, W units a
    subject."""
    S: int
    T: int
    n: int
    L: int
    st: int
    W: int

    def window(self, windowed: bool) -> tuple:
        """(window, stride) as the C calls take them: zeros for whole runs."""
        return (self.L, self.st) if windowed else (0, 0)


def _check_frames(T: int) -> None:
    if T > _FILTER_MAX_FRAMES:
        raise ValueError(f"T = {T} > 2^30 frames: runs this long are not supported")


def _check_timeseries(timeseries, window, stride) -> _Series:
    if not isinstance(timeseries, torch.Tensor):
        raise TypeError(f"timeseries must be a torch.Tensor, got {type(timeseries).__name__}")
    if timeseries.dtype != torch.float32:
        raise TypeError(f"timeseries must be float32, got {timeseries.dtype}")
    for name, v in (("window", window), ("stride", stride)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
            raise TypeError(f"{name} must be an int or None, got {type(v).__name__}")
    if timeseries.dim() != 3 or timeseries.shape[2] == 0:
        raise ValueError(f"timeseries must be [S, T, n] with n >= 1, got {tuple(timeseries.shape)}")
    S, T, n = (int(v) for v in timeseries.shape)
    if T < 2:
        raise ValueError(f"a correlation needs T >= 2 frames, got T = {T}")
    if window is None:
        if stride is not None:
            raise ValueError("stride= is the step between windows: give window= with it")
        L, st = T, T
    else:
        if not 2 <= window <= T:
            raise ValueError(f"window must lie in [2, T] = [2, {T}], got {window}")
        st = window if stride is None else stride
        if st < 1:
            raise ValueError(f"stride must be >= 1, got {st}")
        L = window
    W = (T - L) // st + 1
    if S * W * n >= _LIMIT:
        raise ValueError(f"units * n = {S * W * n} >= 2^31: ingest the cohort in slices of subjects")
    if n * n >= _LIMIT:
        raise ValueError(f"n * n = {n * n} >= 2^31: matrices this large are not supported")
    return _Series(S, T, n, L, st, W)


def _check_run(timeseries) -> _Series:
    """``_check_timeseries`` of whole runs that the filter's kernels take: at most 2^30 frames."""
    series = _check_timeseries(timeseries, None, None)
    _check_frames(series.T)
    return series


def _finite_number(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a float, got {type(v).__name__}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v}")
    return v


def filter_components(T: int, t_r, high_pass=None, low_pass=None) -> tuple:
    """``(k_lo, k_hi)``: the DCT-II components ``k_lo .. k_hi`` of a ``T``-frame run sampled every ``t_r`` seconds that
    the band ``[high_pass, low_pass]`` Hz passes (module docstring); component ``k`` has frequency ``k / (2 T t_r)``.
    ``k_lo - 1 = floor(2 T t_r high_pass)`` is the order of nilearn's and SPM's cosine drift set.  Host only: Python
    floats, no tensor, no device.  ``k_lo > k_hi`` says that the band holds no component."""
    if isinstance(T, bool) or not isinstance(T, int):
        raise TypeError(f"T must be an int, got {type(T).__name__}")
    if T < 2:
        raise ValueError(f"a run has T >= 2 frames, got T = {T}")
    t_r = _finite_number("t_r", t_r)
    if t_r <= 0.0:
        raise ValueError(f"t_r must be > 0, got {t_r}")
    k_lo, k_hi = 1, T - 1
    if high_pass is not None:
        high_pass = _finite_number("high_pass", high_pass)
        if high_pass < 0.0:
            raise ValueError(f"high_pass must be >= 0, got {high_pass}")
        k_lo = math.floor(2 * T * t_r * high_pass) + 1
    if low_pass is not None:
        low_pass = _finite_number("low_pass", low_pass)
        if low_pass <= 0.0:
            raise ValueError(f"low_pass must be > 0, got {low_pass}")
        k_hi = min(T - 1, math.floor(2 * T * t_r * low_pass))
    if high_pass is not None and low_pass is not None and not high_pass < low_pass:
        raise ValueError(f"high_pass must lie below low_pass, got {high_pass} >= {low_pass}")
    return k_lo, k_hi


def _check_out(out, like: torch.Tensor, noun="time series", shape=None) -> None:
    """A valid ``out=``: None, or a float32 contiguous tensor on ``like``'s device, of ``like``'s shape or of ``shape``."""
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a torch.Tensor or None, got {type(out).__name__}")
    if out.dtype != torch.float32:
        raise TypeError(f"out must be float32, got {out.dtype}")
    if tuple(out.shape) != tuple(like.shape if shape is None else shape):
        raise ValueError(f"out must be {tuple(like.shape if shape is None else shape)} as the {noun} are, got "
                         f"{tuple(out.shape)}")
    if out.device != like.device:
        raise ValueError(f"out is on {out.device}, the {noun} on {like.device}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")


def _resident_out(timeseries: torch.Tensor, out) -> torch.Tensor:
    """Where the result of resident time series goes: ``out`` (``_check_out``'s), or a new tensor."""
    _require_resident(timeseries, *_SERIES)
    return torch.empty_like(timeseries) if out is None else out


def _check_confounds(confounds, S=None, T=None, device=None) -> tuple:
    """(S, T, q) of valid confounds; with S, T and device given, of confounds that go with those time series."""
    if not isinstance(confounds, torch.Tensor):
        raise TypeError(f"confounds must be a torch.Tensor, got {type(confounds).__name__}")
    if confounds.dtype != torch.float32:
        raise TypeError(f"confounds must be float32, got {confounds.dtype}")
    if confounds.dim() != 3:
        raise ValueError(f"confounds must be [S, T, q], got {tuple(confounds.shape)}")
    cs, ct, q = (int(v) for v in confounds.shape)
    if S is not None and (cs, ct) != (S, T):
        raise ValueError(f"confounds must be [S, T, q] = [{S}, {T}, q] as the time series are, got "
                         f"{tuple(confounds.shape)}")
    if not 1 <= q <= CONFOUND_MAX:
        raise ValueError(f"confounds hold q = {q} columns: 1 <= q <= CONFOUND_MAX = {CONFOUND_MAX}")
    if ct < 2:
        raise ValueError(f"confounds need T >= 2 frames, got T = {ct}")
    _check_frames(ct)
    if cs >= _LIMIT:
        raise ValueError(f"S = {cs} >= 2^31: ingest the cohort in slices of subjects")
    if device is not None and confounds.device != device:
        raise ValueError(f"confounds are on {confounds.device}, the time series on {device}")
    if not confounds.is_contiguous():
        raise ValueError("confounds must be contiguous")
    return cs, ct, q


def _check_sample_mask(sample_mask, S: int, T: int, device):
    """A valid ``sample_mask=`` for data of ``S`` subjects and ``T`` frames on ``device``: None, or bool ``[S, T]``."""
    if sample_mask is None:
        return None
    if not isinstance(sample_mask, torch.Tensor):
        raise TypeError(f"sample_mask must be a torch.Tensor or None, got {type(sample_mask).__name__}")
    if sample_mask.dtype != torch.bool:
        raise TypeError(f"sample_mask must be bool (True: the frame is kept), got {sample_mask.dtype}")
    if tuple(sample_mask.shape) != (S, T):
        raise ValueError(f"sample_mask must be [S, T] = [{S}, {T}], one flag per frame, got {tuple(sample_mask.shape)}")
    if sample_mask.device != device:
        raise ValueError(f"sample_mask is on {sample_mask.device}, the data on {device}")
    if not sample_mask.is_contiguous():
        raise ValueError("sample_mask must be contiguous")
    return sample_mask


def _masked(name: str, keep) -> tuple:
    """(the entry point of ``name`` that goes with ``keep``, what it takes for the mask)"""
    return (name, ()) if keep is None else (name + "_masked", _lib.buf(keep))


def _confound_basis(confounds: torch.Tensor, keep=None) -> tuple:
    dev = confounds.device
    S, T, q = confounds.shape
    basis = torch.empty(S, T, (q + 31) // 32 * 32, dtype=torch.float32, device=dev)
    rank = torch.empty(S, dtype=torch.int32, device=dev)
    if S:
        name, mask = _masked("cgnn_ingest_confound_basis", keep)
        _call(dev, name, confounds, S, T, q, *mask, *_lib.buf(basis), *_lib.buf(rank))
    return basis, rank


def confound_basis(confounds: torch.Tensor, *, sample_mask=None) -> tuple:
    """``(basis, rank)`` of the confounds float32 ``[S, T, q]``, ``1 <= q <= CONFOUND_MAX``: per subject the orthonormal
    basis of the centred columns by Gram-Schmidt in the given order (module docstring), float32 ``[S, T, qpad]`` with
    ``qpad`` = ``q`` rounded up to 32 -- a column that is constant or that earlier columns explain is exactly zero, as
    the padding is -- and the number of kept columns, int32 ``[S]``; a subject with a non-finite confound has a NaN
    basis and rank -1.  One launch on resident data; no temporaries, no read-back.  ``sample_mask`` (bool ``[S, T]``,
    True: kept) takes every mean, norm and pivot over the subject's kept frames; the rows of the basis at censored
    frames are exactly zero, and a non-finite confound counts only in a kept frame."""
    S, T, q = _check_confounds(confounds)
    keep = _check_sample_mask(sample_mask, S, T, confounds.device)
    _require_resident(confounds, *_CONFOUNDS)
    return _confound_basis(confounds, keep)


def _regress(timeseries: torch.Tensor, basis, out: torch.Tensor, keep=None) -> None:
    """``basis`` None (with ``keep``): masked centring alone."""
    S, T, n = timeseries.shape
    name, mask = _masked("cgnn_ingest_regress", keep)
    _call(timeseries.device, name, timeseries, S, T, n, *mask, *_lib.buf(basis),
          0 if basis is None else int(basis.shape[2]), _WORK, *_lib.buf(out),
          workspace=("cgnn_ingest_regress", S, T, n))


def regress_confounds(timeseries: torch.Tensor, confounds: torch.Tensor, *, sample_mask=None, out=None) -> torch.Tensor:
    """The time series centred and with the span of the subject's centred confounds projected out of every column:
    ``xc - Q (Q^T xc)`` with ``Q = confound_basis(confounds)`` (module docstring), float32 ``[S, T, n]`` on the time
    series' device.  ``confounds`` is float32 contiguous ``[S, T, q]`` on the same device, ``1 <= q <= CONFOUND_MAX``.
    ``out`` as in ``filter_timeseries``: it may be ``timeseries`` itself, with the same bits as out of place.  Three
    launches on resident data; the temporaries are the basis ``[S, T, qpad]`` and the means ``[S, n]``.  No read-back.
    ``sample_mask`` (bool ``[S, T]``, True: kept): the regression runs on the subject's kept frames alone -- the fp64
    least-squares residual of ``x[K]`` on ``[1 | c[K]]`` -- and the censored frames of the result are exactly ``0.0``."""
    S, T = _check_run(timeseries)[:2]
    _check_confounds(confounds, S, T, timeseries.device)
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    _check_out(out, timeseries)
    out = _resident_out(timeseries, out)
    if S:
        _regress(timeseries, _confound_basis(confounds, keep)[0], out, keep)
    return out


def _dropped_components(T: int, k_lo: int, k_hi: int) -> list:
    """What the band ``k_lo .. k_hi`` drops of a ``T``-frame run, ascending."""
    return list(range(1, k_lo)) + list(range(k_hi + 1, T))


def _smaller_set(T: int, k_lo: int, k_hi: int) -> tuple:
    """``(complement, comps)``: whether the set that is multiplied, the smaller one, is what the band drops, and its
    components; refused beyond ``FILTER_MAX_COMPONENTS``."""
    kept = k_hi - k_lo + 1
    dropped = T - 1 - kept
    if min(kept, dropped) > FILTER_MAX_COMPONENTS:
        raise ValueError(f"the band keeps {kept} components and drops {dropped}: the smaller set must hold at most "
                         f"FILTER_MAX_COMPONENTS = {FILTER_MAX_COMPONENTS} (narrow the band, or the part it removes)")
    if kept > dropped:
        return True, _dropped_components(T, k_lo, k_hi)
    return False, list(range(k_lo, k_hi + 1))


def _filter_censored(timeseries: torch.Tensor, k_lo: int, k_hi: int, confounds, keep, out) -> torch.Tensor:
    """``filter_timeseries`` under a mask: the band removed by regression on ``[dropped cosines | confounds]`` at the
    kept frames (module docstring).  The design and its basis are the only temporaries besides the means."""
    S, T, _ = timeseries.shape
    comps = _dropped_components(T, k_lo, k_hi)
    K, nq = len(comps), 0 if confounds is None else int(confounds.shape[2])
    if K + nq > CONFOUND_MAX:
        raise ValueError(f"under a sample_mask the band is removed by regression: it drops {K} components, and with "
                         f"{nq} confound columns that is more than CONFOUND_MAX = {CONFOUND_MAX} regressors (a low_pass "
                         "under censoring would need the censored frames interpolated, which is not built)")
    out = _resident_out(timeseries, out)
    if S == 0:
        return out
    if K + nq == 0:                                   # masked centring: no product launched
        _regress(timeseries, None, out, keep)
        return out
    design = confounds
    if K:
        design = torch.empty(S, T, K + nq, dtype=torch.float32, device=timeseries.device)
        _call(timeseries.device, "cgnn_ingest_design", confounds, S, T, nq, (ctypes.c_int32 * K)(*comps), K,
              *_lib.buf(design))
    basis, _ = _confound_basis(design, keep)
    del design
    _regress(timeseries, basis, out, keep)
    return out


def interpolate_censored(timeseries: torch.Tensor, sample_mask: torch.Tensor, *, out=None) -> torch.Tensor:
    """The time series with every censored frame replaced by a cubic spline through the subject's kept frames, column by
    column (module docstring): float32 ``[S, T, n]`` on the time series' device.  ``timeseries`` is float32 contiguous
    ``[S, T, n]`` on a ROCm device -- confounds ``[S, T, q]`` are served alike -- and ``sample_mask`` bool ``[S, T]``,
    True: kept.  Kept frames are bit copies; what a censored frame holds is never read; inside the kept range the
    spline is ``scipy.interpolate.CubicSpline``'s default (C2, not-a-knot), solved and evaluated in fp64 and rounded to
    fp32 once.  Outside it a censored frame takes the nearest kept value, where ``CubicSpline(extrapolate=True)`` and
    nilearn continue the cubic: over a long censored head or tail that grows without bound and would dominate a
    band-pass.  No kept frame gives zeros, one gives its value everywhere.  ``out`` as in ``filter_timeseries``: it may be
    ``timeseries`` itself, with the same bits as out of place.  Three launches on resident data; the temporary is the
    workspace of the solve (44 bytes per frame and subject, and a slab that depends on the device alone).  No
    read-back, no atomics; every run and every grid gives the same bits."""
    S, T, n = _check_run(timeseries)[:3]
    if sample_mask is None:
        raise TypeError("sample_mask must be a torch.Tensor, got None: interpolate_censored needs the frames to replace")
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    _check_out(out, timeseries)
    out = _resident_out(timeseries, out)
    if S:
        _call(timeseries.device, "cgnn_ingest_interpolate", timeseries, S, T, n, *_lib.buf(keep), _WORK,
              *_lib.buf(out), workspace=("cgnn_ingest_interpolate", S, T, n))
    return out


def _check_order(order) -> int:
    if isinstance(order, bool) or not isinstance(order, int):
        raise TypeError(f"order must be an int, got {type(order).__name__}")
    if not 1 <= order <= BUTTERWORTH_MAX_ORDER:
        raise ValueError(f"order must lie in [1, BUTTERWORTH_MAX_ORDER] = [1, {BUTTERWORTH_MAX_ORDER}], got {order}")
    return order


def butterworth_sos(t_r, high_pass=None, low_pass=None, order=5) -> np.ndarray:
    """The second-order sections, float64 ``[L, 6]`` (``b0 b1 b2 1 a1 a2``, a numpy array), of the digital Butterworth filter of
    that ``order`` for series sampled every ``t_r`` seconds (module docstring): a band-pass of ``order`` sections with
    both bounds, a high-pass (``high_pass`` alone) or a low-pass (``low_pass`` alone) of ``ceil(order / 2)``.  The
    transfer function is ``scipy.signal.butter(order, ..., output="sos", fs=1 / t_r)``'s: the analogue prototype's poles,
    critical frequencies pre-warped, the low-pass to band or high transform, the bilinear transform, conjugate pairs
    into sections; the order of the sections and the pairing are this function's own.  Every section of a high- or
    band-pass has ``b0 + b1 + b2 == 0`` exactly.  Host only: Python floats and ``cmath``, no tensor, no device.  Both
    bounds ``None``, an ``order`` outside ``1 .. BUTTERWORTH_MAX_ORDER`` and a bound outside ``(0, 1 / (2 t_r))`` are
    ``ValueError``s."""
    t_r = _finite_number("t_r", t_r)
    if t_r <= 0.0:
        raise ValueError(f"t_r must be > 0, got {t_r}")
    order = _check_order(order)
    nyquist = 1.0 / (2.0 * t_r)
    if high_pass is None and low_pass is None:
        raise ValueError("a Butterworth filter needs high_pass=, low_pass= or both (filter=\"cosine\" without bounds "
                         "removes the means)")
    bounds = []
    for name, f in (("high_pass", high_pass), ("low_pass", low_pass)):
        if f is None:
            continue
        f = _finite_number(name, f)
        if not 0.0 < f < nyquist:
            raise ValueError(f"{name} must lie in (0, 1 / (2 t_r)), below the Nyquist frequency {nyquist} Hz at "
                             f"t_r={t_r}, got {f}")
        bounds.append(f)
    if len(bounds) == 2 and not bounds[0] < bounds[1]:
        raise ValueError(f"high_pass must lie below low_pass, got {bounds[0]} >= {bounds[1]}")
    # the analogue prototype's poles with a non-negative imaginary part (the others are their conjugates); critical
    # frequencies pre-warped for the bilinear transform at fs = 2, z = (4 + s) / (4 - s)
    proto = [-cmath.exp(1j * math.pi * m / (2 * order)) for m in range(order - 1, 0, -2)]
    if order % 2:
        proto.append(complex(-1.0, 0.0))              # m == 0: the real pole, exactly
    warped = [4.0 * math.tan(math.pi * f / nyquist / 2.0) for f in bounds]
    # the analogue poles of each section: one of a conjugate pair, or the two that the real pole gives a band-pass
    if len(bounds) == 2:
        bw, wo = warped[1] - warped[0], math.sqrt(warped[0] * warped[1])
        groups = []
        for q in proto:
            half = q * bw / 2.0
            root = cmath.sqrt(half * half - wo * wo)
            groups += [(half + root, half - root)] if q.imag == 0.0 else [(half + root,), (half - root,)]
        unit = (4.0 + 1j * wo) / (4.0 - 1j * wo)      # the band's centre, where the gain is 1
    elif high_pass is not None:
        groups = [(warped[0] / q,) for q in proto]
        unit = complex(-1.0, 0.0)                     # the Nyquist frequency
    else:
        groups = [(q * warped[0],) for q in proto]
        unit = complex(1.0, 0.0)                      # frequency 0
    sos = []
    for group in groups:
        z = [(4.0 + q) / (4.0 - q) for q in group]
        if len(z) == 2:                               # two poles, real or each other's conjugates
            a1, a2 = -(z[0] + z[1]).real, (z[0] * z[1]).real
        elif z[0].imag != 0.0:                        # a pole and its conjugate
            a1, a2 = -2.0 * z[0].real, z[0].real ** 2 + z[0].imag ** 2
        else:                                         # the real pole of an odd low- or high-pass: a first-order section
            a1, a2 = -z[0].real, 0.0
        if len(bounds) == 2:
            b = (1.0, 0.0, -1.0)                      # a zero at +1 and one at -1
        else:
            sign = -1.0 if high_pass is not None else 1.0             # zeros at +1 / at -1
            b = (1.0, 2.0 * sign, 1.0) if a2 != 0.0 else (1.0, sign, 0.0)
        # the section's gain: 1 at `unit`.  (b0, b1, b2) stay multiples of small integers by one number, so that a
        # high- or band-pass section has b0 + b1 + b2 == 0 exactly
        u = 1.0 / unit
        g = abs((1.0 + u * (a1 + u * a2)) / (b[0] + u * (b[1] + u * b[2])))
        sos.append([g * b[0], g * b[1], g * b[2], 1.0, a1, a2])
    return np.array(sos, dtype=np.float64)


def _butterworth_edge(sos) -> int:
    """scipy's default pad length of ``sosfiltfilt`` for these sections."""
    L = len(sos)
    return 3 * (2 * L + 1 - min(sum(r[2] == 0.0 for r in sos), sum(r[5] == 0.0 for r in sos)))


def _butterworth(timeseries: torch.Tensor, sos, add_level: bool, out: torch.Tensor) -> None:
    S, T, n = timeseries.shape
    L = len(sos)
    flat = (ctypes.c_double * (6 * L))(*(float(v) for row in sos for v in row))
    _call(timeseries.device, "cgnn_ingest_butterworth", timeseries, S, T, n, flat, L, int(add_level), _WORK,
          *_lib.buf(out), workspace=("cgnn_ingest_butterworth", S, T, n, L))


def _filter_interpolated(timeseries: torch.Tensor, band: dict, confounds, keep, out) -> torch.Tensor:
    """``filter_timeseries(..., sample_mask=, interpolate=True)``: the sequence of public calls of the module docstring."""
    _require_resident(timeseries, *_SERIES)
    out = interpolate_censored(timeseries, keep, out=out)
    filter_timeseries(out, out=out, **band)
    if confounds is None:
        return filter_timeseries(out, t_r=band["t_r"], sample_mask=keep, out=out)
    clean = interpolate_censored(confounds, keep)
    filter_timeseries(clean, out=clean, **band)
    return regress_confounds(out, clean, sample_mask=keep, out=out)


def _filter_butterworth(timeseries, t_r, high_pass, low_pass, order, out, confounds, sample_mask,
                        interpolate: bool) -> torch.Tensor:
    """``filter_timeseries(..., filter="butterworth")``: the checks, then one launch, or the composition around it."""
    S, T, n = _check_run(timeseries)[:3]
    sos = butterworth_sos(t_r, high_pass, low_pass, order)
    edge = _butterworth_edge(sos)
    if T <= edge:
        raise ValueError(f"a Butterworth filter of {len(sos)} sections pads both ends with edge = {edge} mirrored "
                         f"frames (scipy's default): the run must have T > {edge} frames, got T = {T}")
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    if keep is not None and not interpolate:
        raise ValueError("a Butterworth filter is recursive and cannot skip the censored frames of a sample_mask: pass "
                         "interpolate=True, which replaces them first")
    _check_out(out, timeseries)
    if confounds is not None:
        _check_confounds(confounds, S, T, timeseries.device)
    band = dict(t_r=t_r, high_pass=high_pass, low_pass=low_pass, filter="butterworth", order=order)
    if interpolate:
        return _filter_interpolated(timeseries, band, confounds, keep, out)
    out = _resident_out(timeseries, out)
    if S == 0:
        return out
    _butterworth(timeseries, sos, high_pass is None, out)             # a low-pass keeps the level
    if confounds is not None:                         # the same filter on the confounds, then out -= Q (Q^T out) in place
        clean = filter_timeseries(confounds, **band)
        basis, _ = _confound_basis(clean)
        del clean
        _regress(out, basis, out)
    return out


def filter_timeseries(timeseries: torch.Tensor, *, t_r, high_pass=None, low_pass=None, out=None,
                      confounds=None, sample_mask=None, interpolate=False, filter="cosine", order=5) -> torch.Tensor:
    """The time series centred and band-passed column by column, by projection on the DCT-II components
    ``filter_components(T, t_r, high_pass, low_pass)`` of the whole run: float32 ``[S, T, n]`` on the time series'
    device (module docstring), what ``correlation_matrices``, ``ledoit_wolf_shrinkage`` and ``from_timeseries`` take.
    Both bounds ``None`` removes the column means only.  ``out`` is where the result goes: a float32 contiguous tensor
    of the same shape on the same device, which is returned; it may be ``timeseries`` itself (in place, the same bits as
    out of place).  Any other overlap of the two is not checked and gives unspecified values.  Three launches on
    resident data (two without a bound); the temporaries are the basis table ``[T, Kpad]`` and the means ``[S, n]``.
    ``confounds`` (float32 contiguous ``[S, T, q]`` on the same device, ``1 <= q <= CONFOUND_MAX``) are filtered with
    the same band and regressed out of the result in place, ``regress_confounds(filter(timeseries), filter(confounds))``:
    the joint regression on the dropped cosines and the confounds.  The filtered confounds and their basis
    ``[S, T, qpad]`` are its only further temporaries.  No read-back.  ``sample_mask`` (bool ``[S, T]``, True: kept):
    the cosines are not orthogonal on a subset of the frames, so the band is removed by regression,
    ``regress_confounds(timeseries, [dropped cosines | confounds], sample_mask=)``: at most ``CONFOUND_MAX`` regressors
    in all (a ``ValueError`` beyond, which is what a ``low_pass`` usually meets), the censored frames of the result
    exactly ``0.0``; the design ``[S, T, K + q]`` and its basis are then the temporaries.  ``interpolate=True`` (with a
    ``sample_mask``; a ``ValueError`` without one) is the way to a band-pass under censoring, in nilearn's order: the
    censored frames of the series and of the confounds are replaced by ``interpolate_censored``, both are band-passed
    by the orthogonal projection over all ``T`` frames, and the confounds are regressed on the kept frames alone
    (without confounds: the kept frames are centred); exactly that sequence of public calls (module docstring), under
    the checks of the unmasked path, the censored frames of the result exactly ``0.0``.  Its temporaries are the
    interpolated and filtered confounds and their basis, the filter's table and means, and the interpolation
    workspace.  ``filter`` is one of ``FILTERS``.  ``"cosine"``, the default, is all of the above, and ``order`` must
    then be left at its default.  ``"butterworth"`` is nilearn's default instead, a zero-phase Butterworth filter of
    that ``order`` (``1 .. BUTTERWORTH_MAX_ORDER``): every column through ``scipy.signal.sosfiltfilt`` of
    ``butterworth_sos(t_r, high_pass, low_pass, order)`` with scipy's default padding, in fp64 with one rounding to
    fp32 (module docstring); one launch, the same cost for every band and every ``T``, its temporary the slab of
    boundary states (which depends on ``T`` and the device, not on ``S``).  At least one bound is needed, each inside
    ``(0, 1 / (2 t_r))``, and ``T`` must exceed scipy's pad length (33 for the default band-pass).  The result is not
    centred first: a low-pass keeps a column's level.  ``out``, ``confounds`` and ``sample_mask=, interpolate=True``
    are as above with the Butterworth call in the projection's place; a ``sample_mask`` without ``interpolate=True``
    is a ``ValueError``, a recursive filter cannot skip frames."""
    if filter not in FILTERS:
        raise ValueError(f"unknown filter {filter!r}: the filters are FILTERS = {FILTERS}")
    if not isinstance(interpolate, bool):
        raise TypeError(f"interpolate must be a bool, got {type(interpolate).__name__}")
    if interpolate and sample_mask is None:
        raise ValueError("interpolate=True replaces the censored frames: give sample_mask= with it")
    if filter == "butterworth":
        return _filter_butterworth(timeseries, t_r, high_pass, low_pass, order, out, confounds, sample_mask, interpolate)
    if isinstance(order, bool) or order != _BUTTERWORTH_ORDER:
        raise ValueError(f"order={order!r} belongs to filter=\"butterworth\": filter=\"cosine\" takes order="
                         f"{_BUTTERWORTH_ORDER}, its default, only")
    S, T, n = _check_run(timeseries)[:3]
    k_lo, k_hi = filter_components(T, t_r, high_pass, low_pass)
    if k_lo > k_hi:
        raise ValueError(f"the band high_pass={high_pass}, low_pass={low_pass} at t_r={t_r} holds no component of a "
                         f"{T}-frame run (components {k_lo} .. {k_hi}; component k has k / (2 T t_r) Hz)")
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    if keep is None or interpolate:
        complement, comps = _smaller_set(T, k_lo, k_hi)
    _check_out(out, timeseries)
    if confounds is not None:
        _check_confounds(confounds, S, T, timeseries.device)
    if interpolate:
        band = dict(t_r=t_r, high_pass=high_pass, low_pass=low_pass)
        return _filter_interpolated(timeseries, band, confounds, keep, out)
    if keep is not None:
        return _filter_censored(timeseries, k_lo, k_hi, confounds, keep, out)
    out = _resident_out(timeseries, out)
    if S == 0:
        return out
    K = len(comps)                                    # the smaller set is the one that is multiplied
    _call(timeseries.device, "cgnn_ingest_filter", timeseries, S, T, n, (ctypes.c_int32 * K)(*comps), K,
          int(complement), _WORK, *_lib.buf(out), workspace=("cgnn_ingest_filter", S, T, n, K))
    if confounds is not None:                         # the same band on the confounds, then out -= Q (Q^T out) in place
        clean = filter_timeseries(confounds, t_r=t_r, high_pass=high_pass, low_pass=low_pass)
        basis, _ = _confound_basis(clean)
        del clean
        _regress(out, basis, out)
    return out


def series_band(T: int, t_r, band) -> tuple:
    """``(k_lo, k_hi)``: the bins of the DFT of a ``T``-frame run sampled every ``t_r`` seconds that lie in the band
    ``(lo, hi)`` Hz (module docstring); bin ``k`` has frequency ``k / (T t_r)``, ``k = 1 .. K = T // 2``.
    ``k_lo = max(1, ceil(lo T t_r))`` and ``k_hi = min(K, floor(hi T t_r))``: a frequency exactly on a bin is inside.
    Host only: Python floats, no tensor, no device.  ``k_lo > k_hi`` says that the band holds no bin."""
    if isinstance(T, bool) or not isinstance(T, int):
        raise TypeError(f"T must be an int, got {type(T).__name__}")
    if T < 2:
        raise ValueError(f"a run has T >= 2 frames, got T = {T}")
    t_r = _finite_number("t_r", t_r)
    if t_r <= 0.0:
        raise ValueError(f"t_r must be > 0, got {t_r}")
    if not isinstance(band, (tuple, list)) or len(band) != 2:
        raise TypeError(f"band must be a pair (lo, hi) in Hz, got {band!r}")
    lo, hi = _finite_number("band[0]", band[0]), _finite_number("band[1]", band[1])
    if not 0.0 <= lo < hi:
        raise ValueError(f"band must be (lo, hi) with 0 <= lo < hi, got ({lo}, {hi})")
    return max(1, math.ceil(lo * T * t_r)), min(T // 2, math.floor(hi * T * t_r))


def _series_feature_ids(features) -> list:
    if isinstance(features, str):
        features = (features,)
    names = list(features)
    if not names:
        raise ValueError(f"features is empty; choose from SERIES_FEATURES = {SERIES_FEATURES}")
    for name in names:
        if name not in SERIES_FEATURES:
            raise ValueError(f"unknown series feature {name!r}; choose from SERIES_FEATURES = {SERIES_FEATURES}")
    if len(set(names)) != len(names):
        raise ValueError(f"features repeats a name: {names}; each of SERIES_FEATURES = {SERIES_FEATURES} at most once")
    return [SERIES_FEATURES.index(name) for name in names]


def series_features(timeseries: torch.Tensor, *, t_r=None, band=(0.01, 0.08), features=SERIES_FEATURES) -> torch.Tensor:
    """Regional activity features of the series themselves (module docstring): float32 ``[S, n, len(features)]`` on the
    time series' device, the columns in the order of ``features``, any non-empty subset of ``SERIES_FEATURES`` without
    repeats.  What ``node_features=`` of ``from_timeseries`` and ``from_matrices`` takes; with graph measures,
    ``torch.cat`` it with ``node_measures``.  ``t_r`` (seconds) and ``band = (lo, hi)`` in Hz, ``0 <= lo < hi``, are needed
    exactly by the spectral names, those other than ``std`` and ``autocorr1``: the band is the bins
    ``series_band(T, t_r, band)``, and a band without a bin is a ``ValueError``; so is ``T > SERIES_MAX_FRAMES`` with a
    spectral name.  The time series are float32 ``[S, T, n]``, contiguous and resident; they are left untouched, whole
    runs only.  There is no ``sample_mask=``: a censored run goes through ``interpolate_censored`` first, as it does in
    front of a band-pass.  One launch for ``std`` and ``autocorr1``, three with a band, four with ``falff``, which walks
    the whole spectrum (``band_fraction`` is its cheap substitute); the temporaries are the cos/sin table ``[T, 2 bins]``
    and seven doubles per column.  The same bits on every run, for every grid and for every subset or order of names.
    No read-back.  Raises, before any device work: ``ValueError`` for an unknown, repeated or missing name, a missing,
    non-finite or non-positive ``t_r``, a band that is not ``0 <= lo < hi`` or holds no bin, a run too long or not
    ``[S, T, n]``; and, as every time-series call does, ``TypeError`` for series that are not float32 and
    ``RuntimeError`` for series that are not on a ROCm device."""
    ids = _series_feature_ids(features)
    spectral = any(SERIES_FEATURES[i] in _SERIES_SPECTRAL for i in ids)
    S, T, n = _check_run(timeseries)[:3]
    k_lo = k_hi = bins = 0
    if spectral:
        if t_r is None:
            raise ValueError(f"the features {_SERIES_SPECTRAL} are spectral: give t_r= (seconds per frame) with them")
        k_lo, k_hi = series_band(T, t_r, band)
        if k_lo > k_hi:
            raise ValueError(f"the band {tuple(band)} Hz at t_r={t_r} holds no bin of a {T}-frame run (bins {k_lo} .. "
                             f"{k_hi}; bin k has k / (T t_r) Hz, k = 1 .. {T // 2})")
        if T > SERIES_MAX_FRAMES:
            raise ValueError(f"T = {T} > SERIES_MAX_FRAMES = {SERIES_MAX_FRAMES}: the spectral features "
                             f"{_SERIES_SPECTRAL} take runs up to that length; ('std', 'autocorr1') take any")
        # the table's bins: the whole spectrum for falff, else the band from an odd bin on (cgnn_activity.h)
        bins = T // 2 if SERIES_FEATURES.index("falff") in ids else k_hi - ((k_lo - 1) | 1) + 1
    _require_resident(timeseries, *_SERIES)
    out = torch.empty((S, n, len(ids)), dtype=torch.float32, device=timeseries.device)
    if S == 0:
        return out
    _call(timeseries.device, "cgnn_ingest_activity", timeseries, S, T, n, (ctypes.c_int32 * len(ids))(*ids), len(ids),
          k_lo, k_hi, _WORK, *_lib.buf(out), workspace=("cgnn_ingest_activity", S, T, n, bins))
    return out


def _correlate(timeseries: torch.Tensor, series: _Series, windowed: bool, absolute: bool, keep=None) -> tuple:
    """(the correlations [U, n, n], the statistics [U, n, 2] they were built with)"""
    dev = timeseries.device
    S, T, n = series[:3]
    out = torch.empty(S * series.W, n, n, dtype=torch.float32, device=dev)
    stats = torch.empty(S * series.W, n, 2, dtype=torch.float32, device=dev)      # (mean, 1 / sqrt(q)) per unit and ROI
    name, mask = _masked("cgnn_ingest_corr", keep)
    _call(dev, name, timeseries, S, T, n, *series.window(windowed), int(bool(absolute)), *mask, *_lib.buf(stats),
          *_lib.buf(out))
    return out, stats


def _estimate(timeseries: torch.Tensor, series: _Series, windowed: bool, stats: torch.Tensor, matrices: torch.Tensor,
              keep=None) -> torch.Tensor:
    """cgnn_ingest_shrinkage: float64 [U], for the signed correlations and the statistics ``_correlate`` returned."""
    dev = timeseries.device
    S, T, n = series[:3]
    alpha = torch.empty(S * series.W, dtype=torch.float64, device=dev)
    name, mask = _masked("cgnn_ingest_shrinkage", keep)
    inputs = (stats, matrices) if keep is None else _lib.buf(stats) + _lib.buf(matrices)
    _call(dev, name, timeseries, S, T, n, *series.window(windowed), *mask, *inputs, *_lib.buf(alpha))
    return alpha


def _check_shrinkage(shrinkage, units: int, like: torch.Tensor, frames: bool):
    """A valid shrinkage=: a float in [0, 1]; a ``[units]`` tensor on ``like``'s device, as float64 (its values are the
    kernel's to read); or, where the ``frames`` are at hand, a name from SHRINKAGES."""
    if isinstance(shrinkage, torch.Tensor):
        if shrinkage.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"a shrinkage tensor must be float64 (or float32), got {shrinkage.dtype}")
        if tuple(shrinkage.shape) != (units,):
            raise ValueError(f"a shrinkage tensor must be [U] = [{units}], one value per unit, got "
                             f"{tuple(shrinkage.shape)}")
        if shrinkage.device != like.device:
            raise ValueError(f"the shrinkage tensor is on {shrinkage.device}, the data on {like.device}")
        return shrinkage.to(torch.float64).contiguous()
    if isinstance(shrinkage, str) and shrinkage in SHRINKAGES:
        if not frames:
            raise ValueError(f"shrinkage={shrinkage!r} is estimated from the frames, which correlation matrices no "
                             "longer hold: pass shrinkage=ledoit_wolf_shrinkage(timeseries), or ask "
                             "correlation_matrices / from_timeseries for it")
        return shrinkage
    if isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float)):
        got = repr(shrinkage) if isinstance(shrinkage, str) else type(shrinkage).__name__
        raise TypeError(f"shrinkage must be a float, a [U] tensor or one of {SHRINKAGES}, got {got}")
    shrinkage = float(shrinkage)
    if not 0.0 <= shrinkage <= 1.0:                   # (a NaN is refused here too)
        raise ValueError(f"shrinkage must lie in [0, 1], got {shrinkage}")
    return shrinkage


def _check_partial_size(n: int) -> None:
    if n > PARTIAL_MAX_NODES:
        raise ValueError(f"partial correlation takes n <= {PARTIAL_MAX_NODES} nodes (the row panel of a round must "
                         f"fit LDS), got n = {n}")


def _check_kind(kind, shrinkage, n: int, L: int, units: int, timeseries: torch.Tensor):
    """The shrinkage (``_check_shrinkage``'s) of a valid (kind, shrinkage) for ``units`` units of L frames and n ROIs."""
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}: the kinds are {KINDS}")
    shrinkage = _check_shrinkage(shrinkage, units, timeseries, True)
    if kind == "correlation":
        if not isinstance(shrinkage, float) or shrinkage != 0.0:
            raise ValueError('shrinkage applies to kind="partial"; kind="correlation" takes shrinkage=0')
        return shrinkage
    _check_partial_size(n)
    if isinstance(shrinkage, float) and shrinkage == 0.0 and L < n + 2:
        raise ValueError(f"the correlation matrix of {L} frames and n = {n} ROIs is singular by construction (a "
                         f"partial correlation without shrinkage needs at least n + 2 = {n + 2} frames per unit): "
                         "give shrinkage > 0")
    return shrinkage


def _partial(matrices: torch.Tensor, U: int, n: int, shrinkage, absolute: bool, out: torch.Tensor):
    """cgnn_ingest_partial of resident matrices into ``out``, which may be ``matrices``; cgnn_ingest_partial_each if
    ``shrinkage`` is a float64 ``[U]`` tensor.  The workspace is what the query asks for: one slab per workgroup of the
    launch."""
    if U:
        each = isinstance(shrinkage, torch.Tensor)
        _call(matrices.device, "cgnn_ingest_partial_each" if each else "cgnn_ingest_partial", matrices, U, n,
              shrinkage, int(bool(absolute)), _WORK, *_lib.buf(out),
              workspace=("cgnn_ingest_partial", U, n))
    return out


def partial_correlation(matrices: torch.Tensor, *, shrinkage=0.0, absolute=False) -> torch.Tensor:
    """Partial correlation of every unit's correlation matrix: ``[U, n, n]`` float32 on ``matrices.device`` (module
    docstring).  ``matrices`` are read from their upper triangles and left as they are.  One launch on resident data;
    the only temporary is the workspace, one slab per workgroup.  ``shrinkage`` is a float or a ``[U]`` tensor, such as
    ``ledoit_wolf_shrinkage`` gives; the tensor's values are read on the device only.  No read-back."""
    U, n = _check_matrices(matrices)
    shrinkage = _check_shrinkage(shrinkage, U, matrices, False)
    _check_partial_size(n)
    _require_resident(matrices, *_MATRICES)
    return _partial(matrices, U, n, shrinkage, absolute, torch.empty_like(matrices))


def _connectivity(timeseries: torch.Tensor, series: _Series, windowed: bool, absolute: bool, kind: str, shrinkage,
                  keep=None, kendall=False) -> torch.Tensor:
    """The matrices of a valid request: the correlations, or the partial correlations of the signed correlations
    written over them (no second cohort-sized tensor).  A shrinkage named in SHRINKAGES is estimated in between, from
    the frames, the statistics and the signed correlations.  ``kendall``: Kendall's tau-b stands where Pearson's
    correlation does."""
    if kendall:
        signed = kind != "correlation"
        matrices = _kendall(timeseries, series, windowed, keep, absolute and not signed, False, True)[1]
        return _partial(matrices, series.S * series.W, series.n, shrinkage, absolute, matrices) if signed else matrices
    if kind == "correlation":
        return _correlate(timeseries, series, windowed, absolute, keep)[0]
    matrices, stats = _correlate(timeseries, series, windowed, False, keep)
    if isinstance(shrinkage, str):
        shrinkage = _estimate(timeseries, series, windowed, stats, matrices, keep)
    del stats
    return _partial(matrices, series.S * series.W, series.n, shrinkage, absolute, matrices)


def _check_rank(rank, L: int) -> bool:
    """A valid rank= for units of L frames."""
    if not isinstance(rank, bool):
        raise TypeError(f"rank must be a bool, got {type(rank).__name__}")
    if rank:
        _check_rank_frames(L)
    return rank


def _check_rank_frames(L: int) -> None:
    if L > RANK_MAX_FRAMES:
        raise ValueError(f"ranking takes units of at most RANK_MAX_FRAMES = {RANK_MAX_FRAMES} frames (a unit's values "
                         f"and their frame indices must fit LDS), got {L}: rank shorter windows")


def _rank_series(timeseries: torch.Tensor, series: _Series, windowed: bool, keep, out: torch.Tensor) -> torch.Tensor:
    """cgnn_ingest_rank of a valid request on resident data into ``out`` [U, L, n], which without a window may be
    ``timeseries``."""
    S, T, n = series[:3]
    if S:
        name, mask = _masked("cgnn_ingest_rank", keep)
        _call(timeseries.device, name, timeseries, S, T, n, *series.window(windowed), *mask, *_lib.buf(out))
    return out


def _ranked(timeseries: torch.Tensor, series: _Series, windowed: bool, keep) -> tuple:
    """What ``rank=True`` puts in place of a valid request on resident data: (the ranked series ``[U, L, n]``, a new
    tensor; its ``_Series``, whole runs of L frames; its mask ``[U, L]``, the windows of ``keep``)."""
    S, T, n, L, st, W = series
    ranked = torch.empty(S * W, L, n, dtype=torch.float32, device=timeseries.device)
    _rank_series(timeseries, series, windowed, keep, ranked)
    if keep is not None and windowed:
        keep = keep.unfold(1, L, st).reshape(S * W, L).contiguous()
    return ranked, _Series(S * W, L, n, L, L, 1), keep


def rank_timeseries(timeseries: torch.Tensor, *, window=None, stride=None, sample_mask=None, out=None) -> torch.Tensor:
    """The mid-ranks of every column of every unit over the unit's kept frames (module docstring): float32 ``[U, L, n]``
    on the time series' device, ``[S, T, n]`` without a window; the units are ``correlation_matrices``'s.  The Pearson
    correlation of the result is Spearman's rho.  ``sample_mask`` (bool ``[S, T]``, True: kept): the ranks run over the
    unit's kept frames, a censored frame is exactly ``0.0`` and its value is never looked at.  ``out``: without a window
    it may be ``timeseries`` itself, with the same bits; with one it is None or a ``[U, L, n]`` tensor.  A unit has at
    most ``RANK_MAX_FRAMES`` frames.  One launch on resident data, no temporaries, no read-back."""
    series = _check_timeseries(timeseries, window, stride)
    S, T, n, L, _, W = series
    _check_rank_frames(L)
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    if window is None:
        _check_out(out, timeseries)
    else:
        _check_out(out, timeseries, "ranked units", (S * W, L, n))
    _require_resident(timeseries, *_SERIES)
    if out is None:
        out = torch.empty(S * W, L, n, dtype=torch.float32, device=timeseries.device)
    return _rank_series(timeseries, series, window is not None, keep, out)


def _check_kendall(kendall, rank: bool, shrinkage, L: int) -> bool:
    """A valid kendall= beside a valid rank= and a shrinkage that ``_check_kind`` has passed, for units of L frames."""
    if not isinstance(kendall, bool):
        raise TypeError(f"kendall must be a bool, got {type(kendall).__name__}")
    if kendall:
        if rank:
            raise ValueError("kendall=True with rank=True: Kendall's tau is a function of the ranks alone, so the ranked "
                             "call would give the same matrix; leave rank=False")
        if isinstance(shrinkage, str):
            raise ValueError(f"kendall=True with shrinkage={shrinkage!r}: that estimate is a statement about the frames "
                             "of a Pearson correlation matrix; give a float or a [U] tensor")
        _check_kendall_frames(L)
    return kendall


def _check_kendall_frames(L: int) -> None:
    if L > KENDALL_MAX_FRAMES:
        raise ValueError(f"Kendall's tau takes units of at most KENDALL_MAX_FRAMES = {KENDALL_MAX_FRAMES} frames (the "
                         f"keys are twice the mid-ranks in 16 bits and the ranking's own bound is the same), got {L}: "
                         "rank shorter windows")


def _kendall(timeseries: torch.Tensor, series: _Series, windowed: bool, keep, absolute: bool, counts: bool,
             matrices: bool) -> tuple:
    """cgnn_ingest_kendall of a valid request on resident data: (the counts int32 ``[U, n, n]`` or None, tau float32
    ``[U, n, n]`` or None).  The ranked series is the one temporary; without ``counts`` they are formed in the bytes
    of the matrices."""
    ranked, units, _ = _ranked(timeseries, series, windowed, keep)
    U, L, n = units[:3]
    dev = timeseries.device
    g = torch.empty(U, n, n, dtype=torch.int32, device=dev) if counts else None
    tau = torch.empty(U, n, n, dtype=torch.float32, device=dev) if matrices else None
    if U:
        _call(dev, "cgnn_ingest_kendall", ranked, U, L, n, int(bool(absolute)), *_lib.buf(g), *_lib.buf(tau))
    del ranked
    return g, tau


def _kendall_request(timeseries, window, stride, sample_mask) -> tuple:
    """(series, windowed, keep) of a valid request of the two Kendall calls, on resident data."""
    series = _check_timeseries(timeseries, window, stride)
    _check_kendall_frames(series.L)
    keep = _check_sample_mask(sample_mask, series.S, series.T, timeseries.device)
    _require_resident(timeseries, *_SERIES)
    return series, window is not None, keep


def kendall_counts(timeseries: torch.Tensor, *, window=None, stride=None, sample_mask=None) -> torch.Tensor:
    """``G = A^T A`` of every unit (module docstring): int32 ``[U, n, n]`` on the time series' device, the units
    ``correlation_matrices``'s.  ``G_ij`` is concordant minus discordant pairs of kept frames, ``G_ii`` the pairs not
    tied in column ``i``; exact and bit-symmetric.  A unit with fewer than two kept frames is all zeros; a column with a
    NaN in a kept frame has ``G_ii = -1`` and zeros elsewhere in its row and column.  Two launches on resident data (the
    ranking, the counts); the ranked series ``[U, L, n]`` is the one temporary.  ``L <= KENDALL_MAX_FRAMES``."""
    series, windowed, keep = _kendall_request(timeseries, window, stride, sample_mask)
    return _kendall(timeseries, series, windowed, keep, False, True, False)[0]


def kendall_matrices(timeseries: torch.Tensor, *, window=None, stride=None, sample_mask=None,
                     absolute=False) -> torch.Tensor:
    """Kendall's tau-b of the ROI columns of every unit (module docstring): float32 ``[U, n, n]``,
    ``fp32(G_ij / sqrt(G_ii G_jj))`` in fp64 rounded once, ``scipy.stats.kendalltau``.  The diagonal is exactly 1; a
    column that is constant over its kept frames is an exact zero row and column, diagonal included (scipy: NaN); a NaN
    column is NaN in its row and column.  Three launches on resident data (the ranking, the counts written into the
    result's own bytes, the normalisation in place); the ranked series is the one temporary."""
    series, windowed, keep = _kendall_request(timeseries, window, stride, sample_mask)
    return _kendall(timeseries, series, windowed, keep, absolute, False, True)[1]


def _check_labels_and_features(labels, S: int, node_features, letter: str, units: int, n: int) -> None:
    """``labels`` int64 ``[S]``; ``node_features`` None or float32 ``[units, n, F]``, ``letter`` naming the units."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.long or labels.shape != (S,):
        raise ValueError(f"labels must be an int64 tensor [S] = [{S}]")
    if node_features is not None:
        if not isinstance(node_features, torch.Tensor) or node_features.dtype != torch.float32 \
                or node_features.dim() != 3 or tuple(node_features.shape[:2]) != (units, n):
            raise ValueError(f"node_features must be a float32 tensor [{letter}, n, F] = [{units}, {n}, F]")


def ledoit_wolf_shrinkage(timeseries: torch.Tensor, *, window=None, stride=None, sample_mask=None,
                          rank=False) -> torch.Tensor:
    """The Ledoit-Wolf shrinkage of every unit's correlation matrix, estimated from the unit's own frames: float64
    ``[U]`` on the time series' device (module docstring); what ``partial_correlation(..., shrinkage=)`` takes.  Three
    launches on resident data (the two of ``correlation_matrices``, then the estimate); the matrices and the statistics
    are temporaries.  ``n <= PARTIAL_MAX_NODES``.  No read-back.  ``sample_mask`` (bool ``[S, T]``, True: kept): a
    unit's frames are its window's kept ones, ``L_u`` of them, and ``L_u`` stands wherever ``L`` does.  ``rank=True``:
    the estimate for the Spearman matrices, from ``rank_timeseries(timeseries, window=, stride=, sample_mask=)`` (one
    more launch; the ranked series ``[U, L, n]`` is one more temporary, ``W L / T`` times the input with a window)."""
    series = _check_timeseries(timeseries, window, stride)
    _check_partial_size(series.n)
    rank = _check_rank(rank, series.L)
    keep = _check_sample_mask(sample_mask, series.S, series.T, timeseries.device)
    _require_resident(timeseries, *_SERIES)
    windowed = window is not None
    if rank:
        timeseries, series, keep = _ranked(timeseries, series, windowed, keep)
        windowed = False
    matrices, stats = _correlate(timeseries, series, windowed, False, keep)
    return _estimate(timeseries, series, windowed, stats, matrices, keep)


def correlation_matrices(timeseries: torch.Tensor, *, window=None, stride=None, absolute=False, kind="correlation",
                         shrinkage=0.0, sample_mask=None, rank=False, kendall=False) -> torch.Tensor:
    """Pearson correlation of the ROI columns of every unit: ``[U, n, n]`` float32 on the time series' device
    (module docstring).  Two launches on resident data; the only temporary is ``[U, n, 2]`` statistics.
    ``kind="partial"`` gives ``partial_correlation`` of the signed correlations at ``shrinkage``, written in place
    over them by a third launch; ``absolute`` then applies to the partial values.  ``shrinkage`` is a float, a ``[U]``
    tensor or ``"ledoit_wolf"``: each unit's own estimate (``ledoit_wolf_shrinkage``), a launch between the two.
    ``sample_mask`` (bool ``[S, T]``, True: kept): a unit's frames are its window's kept ones; a unit with fewer than
    two is an all-zero matrix.  The ``n + 2`` frames that ``shrinkage == 0`` asks for are still counted on the window:
    kept counts stay on the device, and a unit that its kept frames leave singular is all NaN.
    ``rank=True`` gives Spearman's rank correlation (with ``kind="partial"`` the partial one): bit for bit this call
    without a window on ``rank_timeseries(timeseries, window=, stride=, sample_mask=)`` and the mask's windows
    ``[U, L]``.  One more launch; the ranked series ``[U, L, n]`` is one more temporary -- the size of the input without
    a window, ``W L / T`` times it with one -- freed before the call returns.  ``L <= RANK_MAX_FRAMES``.
    ``kendall=True`` gives Kendall's tau-b, bit for bit ``kendall_matrices(timeseries, ...)``, and with
    ``kind="partial"`` and a float or ``[U]`` shrinkage ``partial_correlation`` of the signed tau matrices (positive
    semidefinite: normalised Gram matrices), written over them.  Not with ``rank=True`` (tau is a function of the ranks
    alone) and not with ``shrinkage="ledoit_wolf"`` (an estimate for Pearson matrices).  ``L <= KENDALL_MAX_FRAMES``."""
    series = _check_timeseries(timeseries, window, stride)
    S, T, n, L, _, W = series
    rank = _check_rank(rank, L)
    shrinkage = _check_kind(kind, shrinkage, n, L, S * W, timeseries)
    kendall = _check_kendall(kendall, rank, shrinkage, L)
    keep = _check_sample_mask(sample_mask, S, T, timeseries.device)
    _require_resident(timeseries, *_SERIES)
    windowed = window is not None
    if rank:
        timeseries, series, keep = _ranked(timeseries, series, windowed, keep)
        windowed = False
    return _connectivity(timeseries, series, windowed, absolute, kind, shrinkage, keep, kendall)


def from_timeseries(timeseries: torch.Tensor, labels: torch.Tensor, *, keep=None, num_edges=None, min_weight=None,
                    window=None, stride=None, absolute=False, node_features=None, measures=None,
                    kind="correlation", shrinkage=0.0, sample_mask=None, knn=None,
                    knn_mode="union", modules=None, backbone=None, group=None, rank=False,
                    kendall=False) -> RaggedPackedDataset:
    """``from_matrices(correlation_matrices(timeseries, ...), labels.repeat_interleave(W), ...)``: one graph per
    unit, every window of a subject carrying the subject's label.  ``labels`` is int64 ``[S]``; ``node_features``,
    if given, is ``[U, n, F]``; a ``min_weight`` tensor is ``[U]``; ``measures`` is ``from_matrices``'s; ``kind`` and
    ``shrinkage`` and ``sample_mask`` are ``correlation_matrices``'s (a unit with fewer than two kept frames is a graph
    without edges).  The one read-back is ``from_matrices``'s.  ``knn=k`` (with ``knn_mode``) instead of the three
    thresholds: the k-NN graph of every unit's matrix, as in ``from_matrices``; the connectivity temporary is sparsified
    in place, which costs no extra memory.  ``modules`` is ``from_matrices``'s.  ``backbone`` is ``from_matrices``'s: the
    connectivity temporary becomes the united graph in place (with ``knn=`` the tree is one more temporary).  ``group``
    is ``from_matrices``'s, its units the windows: the connectivity temporary is masked to the group's edges in place.
    ``rank`` is ``correlation_matrices``'s: Spearman connectivity; the ranked series ``[U, L, n]`` is a temporary beside
    the connectivity one (``W L / T`` times the input with a window) and is freed before the dataset is built.
    ``kendall`` is ``correlation_matrices``'s: Kendall's tau-b connectivity, handed to every edge choice and to
    ``measures=`` unchanged; its ranked temporary is freed before the edges are chosen."""
    series = _check_timeseries(timeseries, window, stride)
    S, T, n, L, _, W = series
    U = S * W
    rank = _check_rank(rank, L)
    shrinkage = _check_kind(kind, shrinkage, n, L, U, timeseries)
    kendall = _check_kendall(kendall, rank, shrinkage, L)
    ids = _check_measures_argument(measures, node_features)
    _check_path_size(ids, n)
    _check_modules_argument(ids, modules, n)
    edges = _edge_plan(n, U, "U", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_labels_and_features(labels, S, node_features, "U", U, n)
    sample_mask = _check_sample_mask(sample_mask, S, T, timeseries.device)
    _require_resident(timeseries, *_SERIES)
    windowed = window is not None
    if rank:
        timeseries, series, sample_mask = _ranked(timeseries, series, windowed, sample_mask)
        windowed = False
    matrices = _connectivity(timeseries, series, windowed, absolute, kind, shrinkage, sample_mask, kendall)
    del timeseries                                    # (the ranked temporary, under rank=True)
    choice = dict(keep=keep, num_edges=num_edges, min_weight=min_weight)       # the caller's, as they came
    if edges.sparsify:
        edges.sparsified(matrices, matrices)
        choice = dict(min_weight=0.0)
    return from_matrices(matrices, labels if W == 1 else labels.repeat_interleave(W), node_features=node_features,
                         measures=measures, modules=modules, **choice)


def _check_knn(n: int, k, mode) -> tuple:
    """``(k, mode id)`` of a valid k-NN request on matrices of ``n`` nodes, as cgnn_ingest_knn takes them."""
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"k must be an int, got {type(k).__name__}")
    if k < 0:
        raise ValueError(f"k must be >= 0, got {k}")
    if not isinstance(mode, str) or mode not in KNN_MODES:
        raise ValueError(f"unknown mode {mode!r}: the modes are KNN_MODES = {KNN_MODES}")
    if n > KNN_MAX_NODES:
        raise ValueError(f"k-NN sparsification takes n <= {KNN_MAX_NODES} nodes (a row lives in 16 registers per "
                         f"lane), got n = {n}")
    return min(k, _LIMIT), _KNN_MODE_IDS[mode]        # anything >= n - 1 keeps every positive entry


def _knn_choice(n: int, knn, knn_mode, keep, num_edges, min_weight):
    """None without ``knn=`` (the call then chooses its edges as it always did); else ``_check_knn``'s pair of a valid
    ``knn=`` / ``knn_mode=``, which goes with none of the three thresholds."""
    if knn is None:
        if knn_mode != "union":
            raise ValueError(f"knn_mode={knn_mode!r} says how the picks of knn= are symmetrised: give knn= with it")
        return None
    if any(a is not None for a in (keep, num_edges, min_weight)):
        raise ValueError("knn= is a fourth way to choose the edges: give none of keep=, num_edges= and min_weight= "
                         "with it")
    return _check_knn(n, knn, knn_mode)


def _check_backbone(n: int, backbone) -> bool:
    """Whether a valid ``backbone=`` asks for the tree on matrices of ``n`` nodes (None: no backbone)."""
    if backbone is None:
        return False
    if not isinstance(backbone, str) or backbone not in BACKBONES:
        raise ValueError(f"unknown backbone {backbone!r}: the backbones are BACKBONES = {BACKBONES}")
    _check_mst_size(n)
    return True


def _check_mst_size(n: int) -> None:
    if n > MST_MAX_NODES:
        raise ValueError(f"the spanning-tree backbone takes n <= {MST_MAX_NODES} nodes (a lane owns 4 nodes of the tree "
                         f"phase), got n = {n}")


def _tree_thresholds(n: int, units: int, unit_name: str, keep, num_edges, min_weight):
    """``_threshold_choice``'s pair of the one threshold a backbone is united with, where none need be given (None: the
    tree alone); two are refused."""
    given = sum(a is not None for a in (keep, num_edges, min_weight))
    if given > 1:
        raise ValueError("the backbone is united with at most one of keep=, num_edges= and min_weight=")
    return _threshold_choice(n, units, unit_name, keep, num_edges, min_weight) if given else None


def _check_statistic(statistic) -> int:
    if not isinstance(statistic, str) or statistic not in GROUP_STATISTICS:
        raise ValueError(f"unknown statistic {statistic!r}: the statistics are GROUP_STATISTICS = {GROUP_STATISTICS}")
    return GROUP_STATISTICS.index(statistic)          # ids: include/cgnn_group.h


def _check_group(n: int, group):
    """A valid ``group=`` for matrices of ``n`` nodes: the id of ``"mean"`` / ``"fisher_mean"``, or the float32
    contiguous ``[n, n]`` tensor it is (whether it lies on the matrices' device is ``_group_of``'s check)."""
    if isinstance(group, torch.Tensor):
        if group.dtype != torch.float32:
            raise TypeError(f"a group tensor must be float32, got {group.dtype}")
        if tuple(group.shape) != (n, n):
            raise ValueError(f"a group tensor must be [n, n] = [{n}, {n}], got {tuple(group.shape)}")
        if not group.is_contiguous():
            raise ValueError("a group tensor must be contiguous")
        return group
    if not isinstance(group, str):
        raise TypeError(f"group must be one of {GROUP_STATISTICS[:2]} or a float32 tensor [n, n], got "
                        f"{type(group).__name__}")
    if group == "consistency":
        raise ValueError('group="consistency" needs a threshold choice of its own, every unit\'s: pass the tensor '
                         'group_matrix(matrices, "consistency", keep=...) as group=')
    return _check_statistic(group)


def _check_among(among, S: int, device):
    """A valid ``among=`` for ``S`` units on ``device``: None, or bool ``[S]``."""
    if among is None:
        return None
    if not isinstance(among, torch.Tensor):
        raise TypeError(f"among must be a torch.Tensor or None, got {type(among).__name__}")
    if among.dtype != torch.bool:
        raise TypeError(f"among must be bool (True: the unit enters the statistic), got {among.dtype}")
    if tuple(among.shape) != (S,):
        raise ValueError(f"among must be [S] = [{S}], one flag per unit, got {tuple(among.shape)}")
    if among.device != device:
        raise ValueError(f"among is on {among.device}, the matrices on {device}")
    if not among.is_contiguous():
        raise ValueError("among must be contiguous")
    return among


def _group(matrices: torch.Tensor, statistic: int, thr=None, among=None) -> torch.Tensor:
    """cgnn_ingest_group of resident matrices: ``[n, n]``; ``thr`` is ``[S]`` exactly for the consistency."""
    S, n = int(matrices.shape[0]), int(matrices.shape[1])
    out = torch.empty(n, n, dtype=torch.float32, device=matrices.device)
    _call(matrices.device, "cgnn_ingest_group", matrices, S, n, statistic, thr, among, _WORK, *_lib.buf(out),
          workspace=("cgnn_ingest_group", S, n))
    return out


def _group_of(matrices: torch.Tensor, group) -> torch.Tensor:
    """The group matrix ``[n, n]`` of ``_check_group``'s value for these resident matrices."""
    if not isinstance(group, torch.Tensor):
        return _group(matrices, group)
    if group.device != matrices.device:
        raise ValueError(f"the group tensor is on {group.device}, the matrices on {matrices.device}")
    return group


class _Edges(NamedTuple):
    """The valid edge choice of a call.  With ``knn`` (``_check_knn``'s pair) or ``tree`` the matrices are sparsified
    first: the k-NN graph, united with the tree if ``tree``; without ``knn`` the tree united with the thresholds of
    ``united`` (``_threshold_choice``'s pair; None: the tree alone).  The call then goes on at ``_threshold_choice``'s
    pair ``(k, min_weight)``, which on sparsified matrices is ``min_weight=0.0``.  With ``group`` -- ``_check_group``'s
    value and the ``_Edges`` of the whole choice for a cohort of one unit -- that choice is made on the group matrix and
    the matrices are sparsified to its edge set; the other fields then say ``min_weight=0.0`` and nothing else."""
    knn: Optional[tuple]
    tree: bool
    united: Optional[tuple]
    k: int
    min_weight: object
    group: Optional[tuple] = None

    @property
    def sparsify(self) -> bool:
        return self.knn is not None or self.tree or self.group is not None

    def sparsified(self, matrices: torch.Tensor, out=None) -> torch.Tensor:
        """The resident matrices sparsified, into ``out`` (which may be ``matrices``) or a new tensor."""
        if self.group is not None:
            group, plan = self.group
            chosen, thr = plan.apply(_group_of(matrices, group)[None])     # (before `out` may overwrite the matrices)
            return _into(matrices, out, "cgnn_ingest_group_mask", chosen, thr)
        if self.knn is None:
            return _mst(matrices, None if self.united is None else _thresholds(matrices, *self.united), out)
        tree = _mst(matrices, None) if self.tree else None            # (before `out` may overwrite the matrices)
        out = _knn(matrices, self.knn, out)
        return out if tree is None else torch.maximum(out, tree, out=out)

    def apply(self, matrices: torch.Tensor, select=True) -> tuple:
        """``(matrices, thr)`` for the caller's matrices, which must be resident and are left as they are: the matrices
        the call goes on with -- sparsified ones are the cohort-sized temporary (two for ``knn=`` with a backbone) --
        and their ``[S]`` thresholds.  Without ``select``, ``thr`` is None where a rank is to be selected: for
        cgnn_ingest_count, which does that with no launch of its own."""
        _require_resident(matrices, *_MATRICES)
        if self.sparsify:
            matrices = self.sparsified(matrices)
        if self.min_weight is None and not select:
            return matrices, None
        return matrices, _thresholds(matrices, self.k, self.min_weight)


def _edge_plan(n: int, units: int, unit_name: str, knn, knn_mode, backbone, keep, num_edges, min_weight,
               group=None) -> _Edges:
    """The ``_Edges`` of a call's whole edge choice: exactly one of the three thresholds; or ``knn=`` with none of
    them; or ``backbone=`` with at most one of them, or with ``knn=``.  With ``group=`` the same choice, for the group
    matrix as a cohort of one unit."""
    if group is not None:
        plan = _edge_plan(n, 1, "the group matrix", knn, knn_mode, backbone, keep, num_edges, min_weight)
        return _Edges(None, False, None, 0, 0.0, (_check_group(n, group), plan))
    choice = _knn_choice(n, knn, knn_mode, keep, num_edges, min_weight)
    tree = _check_backbone(n, backbone)
    if choice is None and not tree:
        return _Edges(None, False, None, *_threshold_choice(n, units, unit_name, keep, num_edges, min_weight))
    united = None if choice is not None else _tree_thresholds(n, units, unit_name, keep, num_edges, min_weight)
    return _Edges(choice, tree, united, 0, 0.0)


def _into(matrices: torch.Tensor, out, name: str, *args) -> torch.Tensor:
    """The launch ``name(matrices, S, n, *args, out, out_bytes)`` of resident matrices, into ``out`` (which may be
    ``matrices``) or a new tensor; ``_WORK`` among ``args`` is the workspace ``name`` asks for, which lives for the call."""
    S, n = int(matrices.shape[0]), int(matrices.shape[1])
    if out is None:
        out = torch.empty_like(matrices)
    if S:
        _call(matrices.device, name, matrices, S, n, *args, *_lib.buf(out),
              workspace=(name, S, n) if any(a is _WORK for a in args) else None)
    return out


def _knn(matrices: torch.Tensor, choice: tuple, out=None) -> torch.Tensor:
    """cgnn_ingest_knn for ``_check_knn``'s pair."""
    return _into(matrices, out, "cgnn_ingest_knn", *choice)


def _mst(matrices: torch.Tensor, thr, out=None) -> torch.Tensor:
    """cgnn_ingest_mst at the ``[S]`` thresholds ``thr`` (None: the tree alone); a slab per workgroup is its workspace."""
    return _into(matrices, out, "cgnn_ingest_mst", thr, _WORK)


def knn_sparsify(matrices: torch.Tensor, k: int, *, mode="union", out=None) -> torch.Tensor:
    """The k-nearest-neighbour graph of every subject as a matrix: float32 ``[S, n, n]`` on ``matrices.device`` with
    the bits of ``matrices`` where an entry is kept and ``+0.0`` elsewhere (module docstring), so that every call of
    this module at ``min_weight=0.0`` sees exactly the k-NN graph.  Every row picks its ``min(k, p_i)`` strongest
    positive off-diagonal entries, ties by the lower column; ``mode`` is one of ``KNN_MODES``: ``"union"`` keeps
    ``i -> j`` if either end picked the other (the usual k-NN graph), ``"mutual"`` if both did, ``"directed"`` the picks
    themselves.  ``k`` is an int ``>= 0``; ``n <= KNN_MAX_NODES``.  ``out`` is where the result goes: a float32 contiguous
    tensor of the same shape on the same device, which is returned; it may be ``matrices`` itself (in place, the same
    bits as out of place; any other overlap is refused).  One launch on resident data (csrc/knn.hip); no temporaries,
    no read-back, no atomics on global memory: every run and every grid gives the same bits."""
    S, n = _check_matrices(matrices)
    choice = _check_knn(n, k, mode)
    _check_out(out, matrices, "matrices")
    _require_resident(matrices, *_MATRICES)
    return _knn(matrices, choice, out)


def mst_backbone(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, out=None) -> torch.Tensor:
    """The maximum-spanning-tree backbone of every subject, united with a threshold, as a matrix: float32 ``[S, n, n]``
    on ``matrices.device`` with the bits of ``matrices`` where an entry is kept and ``+0.0`` elsewhere (module
    docstring), so that every call of this module at ``min_weight=0.0`` sees exactly the united graph.  A positive
    off-diagonal entry is kept iff its pair belongs to the maximum spanning forest of the symmetrised positive weights
    (ties by the lexicographically lower pair: the forest is unique) or the entry lies above the subject's threshold.
    With none of ``keep`` / ``num_edges`` / ``min_weight`` the result is the tree alone; otherwise the thresholds are
    those ``select_thresholds`` or ``from_matrices`` would apply to ``matrices`` for the same choice, of which at most
    one may be given.  What the positive entries connect stays connected: a subject whose positive entries form one
    component gives a connected graph at any density.  ``n <= MST_MAX_NODES``.  ``out`` is where the result goes: a
    float32 contiguous tensor of the same shape on the same device, which is returned; it may be ``matrices`` itself (in
    place, the same bits as out of place; any other overlap is refused).  One launch on resident data (csrc/mst.hip)
    after the selection of the thresholds; the one temporary is the workspace, a matrix-sized slab per workgroup of the
    launch and not per subject; no read-back, no atomics: every run and every grid gives the same bits."""
    S, n = _check_matrices(matrices)
    united = _tree_thresholds(n, S, "S", keep, num_edges, min_weight)
    _check_mst_size(n)
    _check_out(out, matrices, "matrices")
    _require_resident(matrices, *_MATRICES)
    return _Edges(None, True, united, 0, 0.0).sparsified(matrices, out)


def group_matrix(matrices: torch.Tensor, statistic="mean", *, among=None, keep=None, num_edges=None,
                 min_weight=None) -> torch.Tensor:
    """The group-level matrix of a cohort: float32 ``[n, n]`` on ``matrices.device`` (module docstring), what ``group=``
    takes as a tensor.  ``statistic`` is one of ``GROUP_STATISTICS``: ``"mean"``, the entrywise mean over the units;
    ``"fisher_mean"``, ``tanh`` of the mean of ``atanh``; ``"consistency"``, the share of units in which an entry
    survives the unit's own threshold -- exactly one of ``keep`` / ``num_edges`` / ``min_weight`` (a tensor is ``[S]``),
    chosen per unit as ``from_matrices`` would; the other two statistics refuse the three.  ``among`` (``torch.bool``
    ``[S]`` on the device, True: the unit enters the statistic) lets the training split alone define the topology: a
    unit left out is never read, and an all-True ``among`` gives the bits of the call without it.  Sums are fp64 in a
    fixed order, one division, one rounding; no units at all give NaN everywhere.  Two launches on resident data
    (csrc/group.hip; the consistency selects its thresholds first, which reads the cohort once more); the one temporary
    is a workspace ``1 / 32`` of the cohort; no read-back, no atomics: every run and every grid gives the same bits."""
    S, n = _check_matrices(matrices)
    stat = _check_statistic(statistic)
    choice = None
    if statistic == "consistency":
        choice = _threshold_choice(n, S, "S", keep, num_edges, min_weight)
    elif any(a is not None for a in (keep, num_edges, min_weight)):
        raise ValueError(f'keep=, num_edges= and min_weight= are every unit\'s own threshold under "consistency": '
                         f"statistic={statistic!r} takes none of them")
    among = _check_among(among, S, matrices.device)
    _require_resident(matrices, *_MATRICES)
    return _group(matrices, stat, None if choice is None else _thresholds(matrices, *choice), among)


def group_sparsify(matrices: torch.Tensor, group="mean", *, keep=None, num_edges=None, min_weight=None, knn=None,
                   knn_mode="union", backbone=None, out=None) -> torch.Tensor:
    """Every subject masked to one edge set, chosen on a group matrix: float32 ``[S, n, n]`` on ``matrices.device`` with
    the bits of ``matrices`` where an entry is a group edge and positive in the subject, and ``+0.0`` elsewhere (module
    docstring), so that every call of this module at ``min_weight=0.0`` sees the common topology with the subject's own
    weights.  ``group`` is ``"mean"`` or ``"fisher_mean"`` (``group_matrix`` of these matrices), or a float32 contiguous
    ``[n, n]`` tensor on the same device: the way in for ``"consistency"``, which needs a threshold choice of its own and
    is refused as a string, for an ``among=`` split and for a group matrix from elsewhere.  The edge choice -- exactly
    one of ``keep`` / ``num_edges`` / ``min_weight``, or ``knn=`` / ``knn_mode=``, with or without ``backbone="mst"``, as
    in ``from_matrices`` -- is made on the group matrix as a cohort of one unit (a ``min_weight`` tensor is ``[1]``).
    ``out`` is where the result goes: a float32 contiguous tensor of the same shape on the same device, which is
    returned; it may be ``matrices`` itself (in place, the same bits as out of place; any other overlap is refused).  The
    statistic's two launches, the choice's, and one that copies the cohort under the mask (csrc/group.hip); the
    temporaries are group-sized; no read-back, no atomics: every run and every grid gives the same bits."""
    S, n = _check_matrices(matrices)
    if group is None:
        raise TypeError(f"group must be one of {GROUP_STATISTICS[:2]} or a float32 tensor [n, n], got None")
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_out(out, matrices, "matrices")
    _require_resident(matrices, *_MATRICES)
    return edges.sparsified(matrices, out)


def _measure_ids(measures, families=_FAMILIES, what="measures") -> list:
    """A valid request, a non-empty tuple of distinct names of ``families``, as one ``(family, id)`` per column."""
    names = tuple(name for fam in families for name in fam.names)
    if isinstance(measures, str) or not isinstance(measures, (tuple, list)):
        raise TypeError(f"measures must be a tuple of names from {names}, got {measures!r}")
    if len(measures) == 0:
        raise ValueError(f"measures is empty: name at least one of {names}")
    ids = []
    for name in measures:
        entry = next(((fam, fam.names.index(name)) for fam in families if name in fam.names), None)
        if entry is None:
            raise ValueError(f"unknown measure {name!r}: the {what} are {names}")
        if entry in ids:
            raise ValueError(f"measure {name!r} is named twice")
        ids.append(entry)
    return ids


def _check_size(fam: _Family, n: int, subject=None) -> None:
    if fam.max_nodes is not None and n > fam.max_nodes:
        subject = subject or f"the {fam.what} {fam.names} take"
        raise ValueError(f"{subject} n <= {fam.max_nodes} nodes ({fam.why}), got n = {n}")


def _check_path_size(ids, n: int) -> None:
    for fam in _FAMILIES if ids is not None else ():
        if any(f is fam for f, _ in ids):
            _check_size(fam, n)


def _check_measures_argument(measures, node_features):
    """The request of from_matrices's measures= (None: not asked for; True: all of MEASURES)."""
    if measures is None:
        return None
    if node_features is not None:
        raise ValueError("give either measures= or node_features=, not both")
    return _measure_ids(MEASURES if measures is True else measures)


def _check_modules(modules, n: int, device=None) -> tuple:
    """``(labels, M)`` of a valid partition of ``n`` ROIs: ``modules`` is a sequence, a numpy array or a CPU integer
    tensor of ``n`` labels that are exactly ``0 .. M - 1``, each used at least once, ``M <= MODULE_MAX``.  The labels
    come back as a contiguous int32 tensor on ``device`` (None: the host), which is what the kernel trusts.  The whole
    check runs on the host: a device tensor is refused, because checking it would be a read-back."""
    if isinstance(modules, torch.Tensor):
        if modules.device.type != "cpu":
            raise ValueError(f"modules are on {modules.device}: give the partition as a CPU tensor, an array or a "
                             "sequence (its labels are checked on the host; checking a device tensor would be a "
                             "read-back)")
        if modules.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise TypeError(f"modules must hold integer labels, got {modules.dtype}")
        labels = modules.detach().to(torch.int64).numpy()
    else:
        if isinstance(modules, (str, bytes)) or not isinstance(modules, (list, tuple, range, np.ndarray)):
            raise TypeError(f"modules must be a sequence, a numpy array or a CPU integer tensor of n = {n} labels, got "
                            f"{type(modules).__name__}")
        labels = np.asarray(modules)
        if labels.size and (labels.dtype == np.bool_ or not np.issubdtype(labels.dtype, np.integer)):
            raise TypeError(f"modules must hold integer labels, got {labels.dtype}")
        labels = labels.astype(np.int64)
    if labels.shape != (n,):
        raise ValueError(f"modules must be [n] = [{n}] labels, one per ROI, got {tuple(labels.shape)}")
    if int(labels.min()) < 0:
        raise ValueError(f"modules must be labels 0 .. M - 1, got {int(labels.min())}")
    M = int(labels.max()) + 1
    if M > MODULE_MAX:
        raise ValueError(f"modules name M = {M} modules: at most MODULE_MAX = {MODULE_MAX} (a lane of a wave owns one)")
    unused = sorted(set(range(M)) - set(labels.tolist()))
    if unused:
        raise ValueError(f"modules must use every label of 0 .. M - 1 = 0 .. {M - 1}: {unused} have no ROI")
    out = torch.from_numpy(labels.astype(np.int32))
    return (out if device is None else out.to(device)), M


def _check_modules_argument(ids, modules, n: int):
    """``_check_modules``'s pair, on the host, when the request ``ids`` names a module measure (``modules=`` is then
    required), None when it names none (``modules=`` is then refused: it would be ignored)."""
    named = [MODULE_MEASURES[i] for fam, i in (ids or ()) if fam is _MODULES]
    if not named:
        if modules is not None:
            raise ValueError(f"modules= was given but no measure of MODULE_MEASURES = {MODULE_MEASURES} is named")
        return None
    if modules is None:
        raise ValueError(f"the module measures {tuple(named)} need the partition: give modules=, one label per ROI")
    return _check_modules(modules, n)


def _run_family(fam: _Family, matrices: torch.Tensor, thr: torch.Tensor, ids, cols, x, head=(), mid=(), tail=None):
    """One call of ``fam``: measure ``ids[m]`` into column ``cols[m]`` of ``x`` ``[S, n, F]`` (the other columns stay as
    they are; a family without ``cols`` fills ``x`` ``[S, n, len(ids)]`` in the order of ``ids``).  The workspace is what
    the family's query asks for.  What else the C signature of the family takes, as the header lists it: ``head``
    between ``thr`` and the request (``_check_modules``'s pair on the matrices' device), ``mid`` between ``cols, ldx``
    and the workspace (the damping), ``tail`` behind ``x`` (``dist``; ``profile`` and its flags; ``iterations``; each
    pointer with its byte count), by default ``fam.tail``: none of them.  Returns ``x``."""
    S, n = int(matrices.shape[0]), int(matrices.shape[1])
    if S == 0:
        return x
    num = len(ids)
    arr = (ctypes.c_int32 * num)(*ids)
    where = ((ctypes.c_int32 * num)(*cols), x.shape[2] if x is not None else 1) if fam.cols else ()
    _call(matrices.device, fam.call, matrices, S, n, thr, *head, arr, num, *where, *mid, _WORK, *_lib.buf(x),
          *(fam.tail if tail is None else tail), workspace=(fam.call, S, n, arr, num))
    return x


def _run_packed(fam: _Family, matrices: torch.Tensor, thr: torch.Tensor, ids, mid=(), tail=None) -> torch.Tensor:
    """One call of ``fam`` on its own: a new float32 ``[S, n, len(ids)]`` on the matrices' device, column ``m`` holding
    ``ids[m]``.  ``mid`` and ``tail`` are ``_run_family``'s."""
    x = torch.empty(matrices.shape[0], matrices.shape[1], len(ids), dtype=torch.float32, device=matrices.device)
    return _run_family(fam, matrices, thr, ids, list(range(len(ids))), x, mid=mid, tail=tail)


def _measures(matrices: torch.Tensor, S: int, n: int, thr: torch.Tensor, ids: list, modules=None) -> torch.Tensor:
    """``[S, n, len(ids)]``, one call per family that is named.  A request of classic names only is one packed
    cgnn_ingest_measures call, as before; the other families write their columns in place (cols / ldx).  ``modules`` is
    ``_check_modules_argument``'s, on the host."""
    x = torch.empty(S, n, len(ids), dtype=torch.float32, device=matrices.device)
    for fam in _FAMILIES:
        cols = [c for c, (f, _) in enumerate(ids) if f is fam]
        fam_ids = [ids[c][1] for c in cols]
        if not cols:
            continue
        head = (modules[0].to(matrices.device), modules[1]) if fam.modules else ()
        if fam.cols or len(cols) == len(ids):
            _run_family(fam, matrices, thr, fam_ids, cols, x, head)
        else:
            # cgnn_ingest_measures writes a packed block only, so in a mixed request its columns are copied in.  Removing
            # this temporary takes a cols / ldx entry point for the classic family: another change.
            x[:, :, cols] = _run_family(fam, matrices, thr, fam_ids, cols,
                                        torch.empty(S, n, len(cols), dtype=torch.float32, device=matrices.device))
    return x


def node_measures(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None,
                  measures=MEASURES, knn=None, knn_mode="union", modules=None, backbone=None,
                  group=None) -> torch.Tensor:
    """Graph measures of the thresholded matrices as node features: float32 ``[S, n, len(measures)]`` on
    ``matrices.device``, one column per name in ``measures``: names from ``MEASURES``, ``PATH_MEASURES``,
    ``WEIGHTED_PATH_MEASURES`` and ``MODULE_MEASURES`` in any order and mix (module docstring).  The thresholds are
    those ``from_matrices`` applies for the same ``keep`` / ``num_edges`` / ``min_weight``, selected once.  No
    read-back.  ``knn=k`` (with ``knn_mode``) instead of the three: the measures of the k-NN graph, as in
    ``from_matrices``.  ``modules`` is the partition of the ROIs that the names of ``MODULE_MEASURES`` need, and is
    given exactly when one of them is named: a sequence, a numpy array or a CPU integer tensor of ``n`` labels
    ``0 .. M - 1``, each used at least once, ``M <= MODULE_MAX``; one partition for the cohort, checked on the host.
    ``backbone`` is ``from_matrices``'s: the measures of the graph united with the spanning tree.  ``group`` is
    ``from_matrices``'s: the measures of every subject on the group's edge set."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    ids = _measure_ids(measures)
    _check_path_size(ids, n)
    partition = _check_modules_argument(ids, modules, n)
    matrices, thr = edges.apply(matrices)
    return _measures(matrices, S, n, thr, ids, partition)


def module_profile(matrices: torch.Tensor, modules, *, keep=None, num_edges=None, min_weight=None, knn=None,
                   knn_mode="union", binary=False, normalize=False, backbone=None, group=None) -> torch.Tensor:
    """The network profile of every node, the node-to-network feature: float32 ``[S, n, M]`` on ``matrices.device`` with
    ``s_i(m)``, node ``i``'s kept strength into module ``m`` (module docstring), at the thresholds ``from_matrices``
    applies for the same ``keep`` / ``num_edges`` / ``min_weight`` (or on the k-NN graph of ``knn=`` / ``knn_mode=``).
    ``modules`` is ``node_measures``'s partition.  ``binary=True`` gives ``k_i(m)``, the number of kept connections
    into the module; ``normalize=True`` divides a row by its total, an isolated node keeping an exact zero row.  One
    launch (cgnn_ingest_modules without measures); no cohort-sized temporary, no read-back.  With a partition of
    ``M <= 8`` modules (the 7 Yeo networks) the result, passed as ``from_matrices(..., node_features=)``, keeps a
    cohort on the fused GCN path.  ``n <= MODULE_MAX_NODES``.  ``backbone`` is ``from_matrices``'s (the profile of the
    united graph; it and ``knn=`` cost the cohort-sized temporaries named there).  ``group`` is ``from_matrices``'s."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_size(_MODULES, n, "module_profile takes")
    labels, M = _check_modules(modules, n)
    matrices, thr = edges.apply(matrices)
    profile = torch.empty(S, n, M, dtype=torch.float32, device=matrices.device)
    flags = (_lib.MODULE_PROFILE_BINARY if binary else 0) | (_lib.MODULE_PROFILE_NORMALIZE if normalize else 0)
    _run_family(_MODULES, matrices, thr, [], [], None, (labels.to(matrices.device), M), tail=_lib.buf(profile) + (flags,))
    return profile


def _check_damping(damping) -> float:
    if isinstance(damping, bool) or not isinstance(damping, (int, float)):
        raise TypeError(f"damping must be a number, got {type(damping).__name__}")
    if not 0.0 <= damping <= PAGERANK_MAX_DAMPING:    # (a NaN is refused here too)
        raise ValueError(f"damping must lie in [0, {PAGERANK_MAX_DAMPING}], got {damping}")
    return float(damping)


def pagerank_max_steps(damping) -> int:
    """``K_max(d) = ceil(43 ln 2 / -ln d) + 2``, the cap on the steps of ``centrality_measures`` (2 for ``d == 0``).  A
    step is two products, each contracts at rate ``d`` in L1, and the start is at most 2 away: step ``K`` changes by at
    most ``2 (1 + d) d^(2 K - 1)``, below ``2^-84`` at the cap, so the stopping rule ``change <= (1 - d) 2^-42`` holds
    before it in exact arithmetic."""
    d = _check_damping(damping)
    return int(math.ceil(43.0 * math.log(2.0) / -math.log(d))) + 2 if d > 0.0 else 2


def centrality_measures(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, knn=None,
                        knn_mode="union", backbone=None, measures=CENTRALITY_MEASURES, damping=0.85,
                        group=None) -> torch.Tensor:
    """PageRank centrality of the thresholded matrices as node features: float32 ``[S, n, len(measures)]`` on
    ``matrices.device``, one column per name in ``measures``, names from ``CENTRALITY_MEASURES`` in any order (module
    docstring): ``pagerank`` walks the kept entries with equal weights, ``weighted_pagerank`` with the entries' values.
    The edges are those ``node_measures`` sees for the same ``keep`` / ``num_edges`` / ``min_weight`` / ``knn`` /
    ``knn_mode`` / ``backbone``, chosen the same way (``knn=`` and ``backbone=`` cost the cohort-sized temporaries named
    in ``from_matrices``).  ``damping`` is the probability ``d`` of following an edge, a number in
    ``[0, PAGERANK_MAX_DAMPING]``.  Every value is at least ``(1 - d) / n`` and a subject's values sum to 1; an entry
    ``(i, j)`` is an edge ``j -> i`` and a node without out-strength spreads its mass uniformly.  One launch on resident
    data (csrc/pagerank.hip); no workspace, no read-back, no atomics: every run, every grid and every subset and order of
    the names gives the same bits.  ``n <= PAGERANK_MAX_NODES``.  The result is what ``node_features=`` of
    ``from_matrices`` / ``from_timeseries`` takes; its two columns keep a cohort on the fused GCN path.  ``group`` is
    ``from_matrices``'s.

    This is a call of its own beside ``module_profile`` and ``series_features`` and the names are not among those of
    ``node_measures(measures=)``: that table of four families and seventeen names is pinned.  The C entry point writes
    its columns inside a wider ``x`` (cols / ldx) so that a later change can merge the names into ``measures=``."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    ids = [i for _, i in _measure_ids(measures, (_CENTRALITY,), _CENTRALITY.what)]
    damping = _check_damping(damping)
    _check_size(_CENTRALITY, n, "centrality_measures takes")
    matrices, thr = edges.apply(matrices)
    return _run_packed(_CENTRALITY, matrices, thr, ids, mid=(damping,))


def core_measures(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, knn=None, knn_mode="union",
                  backbone=None, measures=CORE_MEASURES, group=None) -> torch.Tensor:
    """The core decomposition of the thresholded matrices as node features: float32 ``[S, n, len(measures)]`` on
    ``matrices.device``, one column per name in ``measures``, names from ``CORE_MEASURES`` in any order (module
    docstring): ``coreness`` is the k-core number over ``n - 1`` (how deep inside the densely connected core a node
    lies; at most its ``degree``), ``onion_layer`` the round of the peeling in which the node leaves, over ``n``, and
    ``s_coreness`` the s-core level over the largest strength (at most its ``strength``).  The edges are those
    ``node_measures`` sees for the same ``keep`` / ``num_edges`` / ``min_weight`` / ``knn`` / ``knn_mode`` /
    ``backbone``, chosen the same way (``knn=`` and ``backbone=`` cost the cohort-sized temporaries named in
    ``from_matrices``).  One launch on resident data (csrc/core.hip); no workspace, no read-back, no atomics: every
    run, every grid and every subset and order of the names gives the same bits.  A kept ``+inf`` makes that subject's
    ``s_coreness`` NaN and nothing else.  ``n <= CORE_MAX_NODES``.  The result is what ``node_features=`` of
    ``from_matrices`` / ``from_timeseries`` takes; its three columns keep a cohort on the fused GCN path.  ``group`` is
    ``from_matrices``'s.

    Like ``centrality_measures`` this is a call of its own and the names are not among those of
    ``node_measures(measures=)``, whose table is pinned."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    ids = [i for _, i in _measure_ids(measures, (_CORE,), _CORE.what)]
    _check_size(_CORE, n, "core_measures takes")
    matrices, thr = edges.apply(matrices)
    return _run_packed(_CORE, matrices, thr, ids)


def core_levels(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, knn=None, knn_mode="union",
                backbone=None, group=None) -> torch.Tensor:
    """The integers behind ``core_measures``: int32 ``[S, n, 3]`` on ``matrices.device`` with the k-core number ``k_i``,
    the onion layer ``r_i`` and the layer ``rho_i`` of the weighted peeling (module docstring), for analyses that want
    them as such -- the members of the 12-core are ``core_levels(m, keep=0.1)[:, :, 0] >= 12``.  A subject with a kept
    ``+inf`` has ``rho_i = -1``.  The edge choice is ``core_measures``'s; one launch, the same kernel, whose three
    float columns are the one temporary.  ``n <= CORE_MAX_NODES``."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_size(_CORE, n, "core_levels takes")
    matrices, thr = edges.apply(matrices)
    levels = torch.empty(S, n, 3, dtype=torch.int32, device=matrices.device)
    _run_packed(_CORE, matrices, thr, list(range(len(CORE_MEASURES))), tail=_lib.buf(levels))
    return levels


def _check_steps(steps) -> list:
    """The ids (``k - 1``) of a valid ``steps=``: an int ``K`` in ``1 .. RW_MAX_STEPS`` stands for ``1, .., K``; else a
    non-empty tuple or list of distinct ints in that range, in any order."""
    def step(k):
        if isinstance(k, bool) or not isinstance(k, int):
            raise TypeError(f"steps must be an int or a tuple of ints in 1 .. {RW_MAX_STEPS}, got {k!r}")
        if not 1 <= k <= RW_MAX_STEPS:
            raise ValueError(f"a step must lie in 1 .. RW_MAX_STEPS = {RW_MAX_STEPS} (steps beyond it need more "
                             f"intermediate products), got {k}")
        return k
    if isinstance(steps, (tuple, list)):
        if len(steps) == 0:
            raise ValueError(f"steps is empty: name at least one of 1 .. {RW_MAX_STEPS}")
        ids = []
        for k in steps:
            if step(k) - 1 in ids:
                raise ValueError(f"step {k} is named twice")
            ids.append(k - 1)
        return ids
    return list(range(step(steps)))


def random_walk_encodings(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, knn=None,
                          knn_mode="union", backbone=None, group=None, steps=RW_MAX_STEPS,
                          binary=False) -> torch.Tensor:
    """The random-walk structural encoding of the thresholded matrices as node features (RWSE; PyG's
    ``AddRandomWalkPE`` on a symmetric kept set): float32 ``[S, n, len(steps)]`` on ``matrices.device``, the column of
    step ``k`` holding ``((P)^k)_ii``, the probability that a ``k``-step walk from node ``i`` is back at ``i``, with
    ``P`` the row-normalised kept weights (module docstring; ``binary=True`` walks the kept entries with equal weights).
    ``steps`` is an int ``K`` in ``1 .. RW_MAX_STEPS`` for the steps ``1, .., K``, or a tuple of distinct steps in any
    order, one column each.  The edges are those ``node_measures`` sees for the same ``keep`` / ``num_edges`` /
    ``min_weight`` / ``knn`` / ``knn_mode`` / ``backbone``, chosen the same way (``knn=`` and ``backbone=`` cost the
    cohort-sized temporaries named in ``from_matrices``).  One launch on resident data (csrc/rw.hip); the intermediate
    products live in a workspace of one slab set per workgroup, whatever ``S`` is; no read-back, no atomics: every run,
    every grid and every subset and order of the steps gives the same bits.  Every value lies in ``[0, 1]``; step 1 is
    exactly 0; a kept ``+inf`` makes that subject's columns for ``k >= 2`` NaN and nothing else.
    ``n <= RW_MAX_NODES``.  The result is what ``node_features=`` of ``from_matrices`` / ``from_timeseries`` takes; the
    default eight columns are exactly those that keep a cohort on the fused GCN path.  ``group`` is ``from_matrices``'s.

    Like ``centrality_measures`` and ``core_measures`` this is a call of its own, not a name of
    ``node_measures(measures=)``, whose table is pinned."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    ids = _check_steps(steps)
    if not isinstance(binary, bool):
        raise TypeError(f"binary must be a bool, got {type(binary).__name__}")
    _check_size(_RW, n, "random_walk_encodings takes")
    matrices, thr = edges.apply(matrices)
    return _run_packed(_RW, matrices, thr, ids, mid=(_lib.RW_BINARY if binary else 0,))


def path_lengths(matrices: torch.Tensor, *, keep=None, num_edges=None, min_weight=None, knn=None,
                 knn_mode="union", backbone=None, group=None) -> torch.Tensor:
    """The weighted distances ``dw`` of the module docstring: float32 ``[S, n, n]`` on ``matrices.device``, ``+inf``
    where ``j`` is not reached from ``i`` and a zero diagonal, at the thresholds ``from_matrices`` applies for the same
    ``keep`` / ``num_edges`` / ``min_weight``.  This is the one call of this module whose output is cohort-sized: as
    large as ``matrices`` itself.  The measures of ``WEIGHTED_PATH_MEASURES`` are formed from the same distances without
    it (``node_measures``).  ``n <= WEIGHTED_PATH_MAX_NODES``.  No read-back.  ``knn=k`` (with ``knn_mode``) instead of
    the three: the distances on the k-NN graph, as in ``from_matrices``.  ``backbone`` is ``from_matrices``'s: on a
    subject whose positive entries form one component every distance is then finite.  ``group`` is ``from_matrices``'s."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_size(_WEIGHTED, n, "path_lengths takes")
    matrices, thr = edges.apply(matrices)
    dist = torch.empty(S, n, n, dtype=torch.float32, device=matrices.device)
    _run_family(_WEIGHTED, matrices, thr, [], [], None, tail=_lib.buf(dist))
    return dist


def select_thresholds(matrices: torch.Tensor, *, keep=None, num_edges=None) -> torch.Tensor:
    """Per subject, the off-diagonal entry of descending rank ``k`` (``[S]`` float32 on the matrices'
    device): the threshold that ``from_matrices`` applies for the same ``keep`` / ``num_edges``."""
    _, n = _check_matrices(matrices)
    k = _rank(n, keep, num_edges)
    _require_resident(matrices, *_MATRICES)
    return _thresholds(matrices, k, None)


def from_matrices(matrices: torch.Tensor, labels: torch.Tensor, *, keep=None, num_edges=None, min_weight=None,
                  node_features=None, measures=None, knn=None, knn_mode="union",
                  modules=None, backbone=None, group=None) -> RaggedPackedDataset:
    """The thresholded cohort as a ``RaggedPackedDataset`` on ``matrices.device`` (module docstring).  With
    ``measures`` (a tuple of names from ``MEASURES``, ``PATH_MEASURES``, ``WEIGHTED_PATH_MEASURES`` and
    ``MODULE_MEASURES``, or ``True`` for all of ``MEASURES``) ``x`` is ``node_measures`` at the thresholds of this call,
    which are selected once; ``modules`` is ``node_measures``'s partition, given exactly when a module measure is named.

    One synchronisation: the ``S + 1`` edge offsets are read back once, to size the edge arrays and to fill
    the host ``edge_ptr`` the dataset carries; ``edge_ptr_dev`` is the array the kernels' running sum left.

    ``knn=k`` is a fourth way to choose the edges, given instead of ``keep`` / ``num_edges`` / ``min_weight``: the
    k-nearest-neighbour graph, symmetrised as ``knn_mode`` (one of ``KNN_MODES``) says.  The call is, bit for bit, this
    call on ``knn_sparsify(matrices, k, mode=knn_mode)`` with ``min_weight=0.0``: the strength feature and every
    measure are those of the k-NN graph.  The caller's matrices are left as they are, so the sparsified cohort is a
    temporary as large as ``matrices`` for the length of the call (``node_measures`` and ``path_lengths`` alike); a
    caller who can give the matrices up passes ``knn_sparsify(m, k, out=m)`` and ``min_weight=0.0`` instead.

    ``backbone="mst"`` (one of ``BACKBONES``) unites the chosen edges with the maximum spanning forest of the positive
    weights, so that whatever the positive entries connect stays connected at any density.  With one of ``keep`` /
    ``num_edges`` / ``min_weight`` the call is, bit for bit, this call on ``mst_backbone(matrices, <that choice>)`` with
    ``min_weight=0.0``, the thresholds being those of the original matrices; alone (only then may the three be left out)
    it is the tree alone; with ``knn=`` it is this call on ``torch.maximum(knn_sparsify(matrices, k, mode=knn_mode),
    mst_backbone(matrices))`` with ``min_weight=0.0``, which needs two cohort-sized temporaries for the length of the
    call, the k-NN graph and the tree (the other choices need one, the united graph).  The strength feature and every
    measure are those of the united graph, which has at most ``2 (n - 1)`` more entries than the choice alone.  Any
    other value raises a ``ValueError`` naming ``BACKBONES``.

    ``group=`` changes whose matrix that whole choice is made on: ``"mean"``, ``"fisher_mean"`` or a float32 ``[n, n]``
    tensor on the matrices' device (``group_matrix``'s, which is the way in for ``"consistency"`` and for an ``among=``
    split).  The choice above, thresholds, ``knn=`` and ``backbone=`` alike, is applied to the group matrix as a cohort
    of one unit (a ``min_weight`` tensor is ``[1]``) and every subject carries that edge set with its own weights: the
    call is, bit for bit, this call on ``group_sparsify(matrices, group, <the choice>)`` with ``min_weight=0.0``.  A
    subject whose entry at a group edge is not positive drops that edge.  The masked cohort is the one cohort-sized
    temporary."""
    S, n = _check_matrices(matrices)
    edges = _edge_plan(n, S, "S", knn, knn_mode, backbone, keep, num_edges, min_weight, group)
    _check_labels_and_features(labels, S, node_features, "S", S, n)
    if node_features is not None and node_features.device != matrices.device:
        raise ValueError(f"node_features are on {node_features.device}, the matrices on {matrices.device}")
    ids = _check_measures_argument(measures, node_features)
    _check_path_size(ids, n)
    partition = _check_modules_argument(ids, modules, n)
    matrices, thr = edges.apply(matrices, select=False)
    dev = matrices.device
    select = thr is None                              # cgnn_ingest_count selects them: no launch of its own
    if select:
        thr = torch.empty(S, dtype=torch.float32, device=dev)
    row_count = torch.empty(S * n, dtype=torch.int32, device=dev)
    strength = None                                   # the default feature, unless x comes from elsewhere
    if node_features is None and ids is None:
        strength = torch.empty(S, n, 1, dtype=torch.float32, device=dev)
    x = node_features if node_features is not None else strength
    row_off = torch.zeros(S * n + 1, dtype=torch.long, device=dev)
    with _lib.device_guard(dev):
        sp = _lib.stream_ptr(dev)
        _lib.call("cgnn_ingest_count", matrices, S, n, int(select), edges.k, *_lib.buf(thr), *_lib.buf(row_count),
                  *_lib.buf(strength), stream=sp)
        torch.cumsum(row_count, 0, dtype=torch.long, out=row_off[1:])
        edge_ptr_dev = row_off[::n].contiguous()          # [S + 1]: every subject's first row
        edge_ptr = edge_ptr_dev.cpu()                     # the one read-back
        E = int(edge_ptr[-1])
        edge_local = torch.empty(2, E, dtype=torch.long, device=dev)
        edge_weight = torch.empty(E, dtype=torch.float32, device=dev)
        _lib.call("cgnn_ingest_fill", matrices, S, n, thr, row_off, E, *_lib.buf(edge_local), *_lib.buf(edge_weight),
                  stream=sp)
    if ids is not None:
        x = _measures(matrices, S, n, thr, ids, partition)        # at the thresholds cgnn_ingest_count selected
    return RaggedPackedDataset(x, edge_local, edge_weight, labels.to(dev), edge_ptr, edge_ptr_dev)
