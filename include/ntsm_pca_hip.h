/*
 * include/ntsm_pca_hip.h -- C ABI of the MI355X (gfx950) device steps of ntsmPCA: the exact PCA of the matrix that
 * `ntsmVCF -p NAME` writes (NAME_matrix.tsv), i.e. the rotation that `ntsmEval -p` reads.
 *
 * With A the p x n matrix of the file (p sites, n samples; host, row-major, IEEE double), c_j the mean of row j and
 * Ac = A - c:
 *   G = Ac^T Ac (n x n);  (l_i, u_i) its D largest eigenpairs, descending;  s_i = sqrt(l_i);
 *   rotation column i:  v_i = Ac u_i / s_i (length p);   scores of the samples:  t_i = s_i u_i (length n);
 *   sign: the entry of v_i with the largest absolute value (the first one on a tie) is positive, t_i follows.
 * This is what sklearn.decomposition.PCA(n_components=D, svd_solver="full") computes on A^T (components_ transposed and
 * the transformed samples), up to rounding.
 *
 * Device steps: (1) row means in a fixed order, Ac written once over the uploaded copy of A (zero padded to the tile
 * sizes); (2) the Gram product with v_mfma_f64_16x16x4_f64, upper 128 x 128 tiles only, the site dimension split over
 * workgroups and the partial tiles summed by a second kernel in split order, mirrored into the lower triangle; (3) the
 * eigenpairs of G with rocSOLVER's dsyevd (bound with dlopen on first use); (4) V = Ac U_D / s and T = U_D s.
 * No floating-point atomics anywhere: every result is a pure function of the input and of `split`.
 *
 * The matrix may also be given as the 16-bit cells of ntsm_vcf_run (include/ntsm_vcf_hip.h) with the value of every cell
 * code, the form `ntsmVCF --rotation` hands over: the *_cells entry points below.  The doubles then exist on the device
 * only: step (0), ntsm_pca_expand, writes the whole padded buffer from the cells, and steps (1) to (4) follow unchanged.
 *
 * Or as the first n records of a cohort store (`ntsmPCA --store`): the *_store entry points at the
 * end.  The cells are then made on the device from the store's counts, chunk by chunk, and never cross the host.
 */
#ifndef NTSM_PCA_HIP_H
#define NTSM_PCA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntsm_pca_times {     /* milliseconds; upload / download wall clock, device steps from HIP events */
	double upload_ms, centre_ms, gram_ms, eigen_ms, project_ms, download_ms;
	uint64_t gram_flops;             /* n (n + 1) p: the multiply-adds of the triangle, counted as two operations each */
	uint64_t gram_bytes;             /* bytes the Gram kernels read and write at least once (panels, partial tiles, G) */
	uint32_t gram_tiles, gram_split; /* upper 128 x 128 tiles; pieces the site dimension was cut into */
} ntsm_pca_times;

enum {
	NTSM_PCA_E_ARG = -1,             /* bad argument */
	NTSM_PCA_E_HIP = -2,             /* HIP error (text on stderr) */
	NTSM_PCA_E_SOLVER_MISSING = -3,  /* librocsolver.so.0 / librocsolver.so could not be loaded or lacks a symbol */
	NTSM_PCA_E_SOLVER = -4,          /* rocSOLVER returned an error or dsyevd did not converge */
	NTSM_PCA_E_RANK = -5             /* a requested component's eigenvalue is <= n * eps * l_1; *bad_component says which */
};

/*
 * The Gram step on its own.
 * a:       host [p][n] row-major.
 * centre:  non-zero: G = Ac^T Ac; 0: G = A^T A (the row means are still computed when `means` is given).
 * split:   pieces of the site dimension; 0 = chosen from p, n and the device's compute units.  Clamped to the number
 *          of 16-site chunks.
 * gram:    host out [n][n], symmetric (the lower triangle is the mirror of the upper one, bit for bit).
 * means:   host out [p], may be NULL.
 * times:   may be NULL.
 */
int ntsm_pca_gram(int device, uint64_t p, uint32_t n, const double *a, int centre, uint32_t split,
		double *gram, double *means, ntsm_pca_times *times);

/*
 * The whole PCA.  1 <= d <= min(n, p), n >= 2.
 * eigval:  host out [d], descending.
 * rot:     host out [p][d] (row = site, the layout of NAME_rotationalMatrix.tsv).
 * comp:    host out [n][d] (row = sample, the layout of NAME_components.tsv).
 * bad_component: out, set with NTSM_PCA_E_RANK; may be NULL.
 */
int ntsm_pca_run(int device, uint64_t p, uint32_t n, const double *a, uint32_t d, uint32_t split,
		double *eigval, double *rot, double *comp, uint32_t *bad_component, ntsm_pca_times *times);

/*
 * The matrix as cells.  Cell (s, j) of the p x n matrix is
 *   code = cells[s * n + j] != 0:  value[0][code] where s * n + j <= first_undef_cell, value[1][code] after it;
 *   code = 0:                      row_fill[s].
 * cells:    host [p][n] row-major, as ntsm_vcf_run returns them (maxREF | maxVAR << 8).
 * value:    host [2][65536] doubles; the caller fills the entries of every code that occurs, entry 0 of both halves is
 *           not read.  (ntsmVCF fills them with what ntsmPCA would read back from the two texts a code is printed as.)
 * row_fill: host [p] doubles.
 * first_undef_cell: a linear index s * n + j, compared in 64 bits; ~0 for none (value[1] is then not read).
 * expand_ms: out, may be NULL: the expansion kernel's time from HIP events.  times->upload_ms is the upload of cells,
 *           table and fills.
 * Argument checks, return codes and `times` are those of the entry points above.
 *
 * Contract: ntsm_pca_run_cells(...) returns the same bits as ntsm_pca_run on the matrix ntsm_pca_expand_cells(...)
 * returns, and ntsm_pca_gram_cells the same bits as ntsm_pca_gram on it -- for the same `split`, in the same process
 * (the same rocSOLVER build).
 */

/* The expansion on its own.  a: host out [p][n] row-major (the padding of the device buffer is not returned; that it is
 * zero shows in G). */
int ntsm_pca_expand_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, double *a /* host out [p][n] */, double *expand_ms);

/* ntsm_pca_gram on the cells: the test hook for the padding the expansion writes */
int ntsm_pca_gram_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, int centre, uint32_t split, double *gram, double *means,
		ntsm_pca_times *times, double *expand_ms);

/* ntsm_pca_run on the cells */
int ntsm_pca_run_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, uint32_t d, uint32_t split,
		double *eigval, double *rot, double *comp, uint32_t *bad_component, ntsm_pca_times *times, double *expand_ms);

/*
 * The matrix from a cohort store: the genotypes that ntsmEval's projection derives from the counts
 * of the store's samples, with every site centred over the samples that call it.
 *
 * db_counts: host; the counts of sample j, uint32 [n_sites][2] (AT, CG), at db_counts + j * db_stride_bytes -- a mapped
 *            store's records (host/eval_store.hpp), or any buffer of that pitch.  db_stride_bytes >= 8 * n_sites, a
 *            multiple of 4.
 * n:         samples taken, the first n records.  p of the entry points above is n_sites.
 * min_cov:   a count at or below it reads as 0 (ntsmEval -c).
 * db_chunk:  samples uploaded per pass; 0 = as many as fit in half of the free device memory.
 * The cell of (site s, sample j) is code + 1 with code the genotype code of the two counts (0 / 1 / 2 for genotype
 * 0 / 0.5 / 1), and 0 where the sample does not call the site.  tallies[s] = { n_half, n_one, n_called }: the samples of
 * genotype 0.5, of genotype 1, and all that call the site.  The value table of the cells is value[0][1..3] = { 0, 0.5, 1 },
 * first_undef_cell = ~0, and row_fill[s] is what ntsmPCA reads back from the text of (n_one + 0.5 n_half) / n_called as
 * NAME_center.txt holds it ("0" where n_called = 0): host/pca_text.hpp, store_centre_text.
 *
 * Contract: ntsm_pca_run_store(...) returns the same bits as ntsm_pca_run_cells on the cells ntsm_pca_store_cells returned
 * with that table and those fills -- for the same `split`, in the same process, for every db_chunk.  Cells and tallies
 * are integers (the tallies summed with integer atomics), so they do not depend on db_chunk or on the order of anything.
 * Argument checks and return codes are those of the entry points above.
 */
typedef struct ntsm_pca_store_times {   /* milliseconds */
	double upload_ms;                    /* the 2-D copies of the chunks' counts, wall clock */
	double genotype_ms;                  /* the genotype kernel over all chunks, HIP events */
	double fill_ms;                      /* tallies down, centre texts and fills on the host, fills and value table up: wall clock */
	double expand_ms;                    /* ntsm_pca_expand, HIP events (ntsm_pca_run_store only) */
	uint32_t chunks, chunk;              /* passes, and samples per pass */
} ntsm_pca_store_times;

/* The genotype step on its own.  cells: host out [n_sites][n] row-major; tallies: host out [n_sites][3]. */
int ntsm_pca_store_cells(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n, uint64_t n_sites, uint32_t min_cov,
		uint32_t db_chunk, uint16_t *cells, uint32_t *tallies, ntsm_pca_store_times *store_times);

/* The whole PCA of a store's first n samples; eigval, rot, comp, bad_component, times as ntsm_pca_run.  times->upload_ms is
 * store_times->upload_ms.  tallies: host out [n_sites][3]; store_times: may be NULL. */
int ntsm_pca_run_store(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n, uint64_t n_sites, uint32_t min_cov,
		uint32_t db_chunk, uint32_t d, uint32_t split, double *eigval, double *rot, double *comp, uint32_t *tallies,
		uint32_t *bad_component, ntsm_pca_times *times, ntsm_pca_store_times *store_times);

#ifdef __cplusplus
}
#endif
#endif
