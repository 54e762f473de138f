// Package main (drop-in file for DistributedML/Biscotti DistSys/).
//
// krum_bk.go replaces the go-python Multi-Krum call of DistSys/krum.go with the
// MI355X engine libbk.so (include/bk.h).  It keeps the verifier call surface:
//
//	func (krumval *KRUMValidator) initialize()                        krum.go:31-44
//	func (krumval *KRUMValidator) getTopKRUMIndex(deltas [][]float64) []int
//	                                                                  krum.go:100-166
//
// computeScores (krum.go:77-98), VerifyUpdateKRUM (:227-365),
// startKRUMDeadlineTimer (:178-224) and checkIfAccepted (:47-73) are unchanged.
// To adopt it: delete getTopKRUMIndex/initialize (and the pyKRUMFunc global)
// from krum.go, add this file, build with
//
//	CGO_CFLAGS="-I<repo>/include" CGO_LDFLAGS="-L<repo>/biscotti_amd -lbk -Wl,-rpath,<repo>/biscotti_amd" go build
//
// NOT BUILT IN THIS REPOSITORY: the build image has no Go toolchain (see
// INTEGRATION.md).  The C calls it makes are exercised from Python through the
// same ABI (tests/test_abi.py, tests/test_gpu_parity.py).
package main

/*
#cgo LDFLAGS: -lbk
#include <stdlib.h>
#include <string.h>
#include "bk.h"

// bk_shares_recover's pointer table is `const int64_t *const *`; the table is
// C-allocated (void *), so the cast is made here
static int sharesRecoverC(bk_ctx *ctx, void *parts, const int *held, const int64_t *xs, int nparts,
                          int where, int64_t d, int poly_size, int precision,
                          const double *global_w, int64_t *coef_out, double *delta_out,
                          double *global_out, int64_t *bad_chunks) {
    return bk_shares_recover(ctx, (const int64_t *const *)parts, held, xs, nparts, where, d,
                             poly_size, precision, global_w, coef_out, delta_out, global_out,
                             bad_chunks);
}
*/
import "C"

import (
	"os"
	"runtime"
	"strconv"
	"unsafe"

	"github.com/dedis/kyber"
)

var (
	bkCtx      *C.bk_ctx   // device 0's context (the group's rank 0 when bkGroup is set)
	bkGroup    *C.bk_group // BK_GPUS > 1: one process driving that many GPUs
	bkStage    unsafe.Pointer // C-owned pinned staging (cgo may not keep Go pointers)
	bkStageLen int64
)

// initialize binds the engine instead of pyKRUMFunc (krum.go:31-44).  With
// BK_GPUS=G (G > 1) the verifier drives G GPUs from this one process: each
// copies its column shard of the batch over its own PCIe link (bk_group_*).
func (krumval *KRUMValidator) initialize() {
	if bkCtx != nil {
		return
	}
	if g, err := strconv.Atoi(os.Getenv("BK_GPUS")); err == nil && g > 1 {
		var grp *C.bk_group
		if st := C.bk_group_create(&grp, C.int(g), nil, C.BK_GROUP_ALLREDUCE); st != C.BK_OK {
			outLog.Printf("bk_group_create(%d) failed (%d): %s", g, int(st),
				C.GoString(C.bk_last_error()))
			return
		}
		bkGroup, bkCtx = grp, C.bk_group_ctx(grp, 0)
		outLog.Printf("Krum engine: libbk ABI %d on %d GPUs", int(C.bk_abi_version()), g)
		return
	}
	var ctx *C.bk_ctx
	if st := C.bk_create(&ctx, 0); st != C.BK_OK {
		outLog.Printf("bk_create failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return
	}
	bkCtx = ctx
	outLog.Printf("Krum engine: libbk ABI %d", int(C.bk_abi_version()))
}

// getTopKRUMIndex keeps the signature and the clip rule of krum.go:100-166:
// adversaryCount := int(NumAdversaries * float64(n)); the accepted indices
// index the (SourceID-sorted) UpdateList.  They come back ascending -- the
// reference returned numpy argpartition order, and its only consumer,
// checkIfAccepted, tests membership.  On any engine error every update is
// rejected (empty list), which is what a failing Python call led to.
//
// The rows go to libbk as they are (bk_multikrum_rows): a C array of the n
// row pointers, each row's backing array pinned for the call -- Go pointers
// stored in C memory, legal while pinned (runtime.Pinner, Go >= 1.21).  libbk
// packs them into its own pinned memory on host threads, each column chunk's
// H2D and Gram starting as soon as it is packed, instead of this goroutine
// copying all n rows into a pinned batch first (the old serial pack, kept
// for the multi-GPU group below).
func (krumval *KRUMValidator) getTopKRUMIndex(deltas [][]float64) []int {
	n := len(deltas)
	if n == 0 || bkCtx == nil {
		return []int{}
	}
	d := len(deltas[0])
	f := int(krumval.NumAdversaries * float64(n))
	if C.bk_check_args(C.int64_t(n), C.int64_t(d), C.int64_t(f)) != C.BK_OK {
		outLog.Printf("Krum: %s", C.GoString(C.bk_last_error()))
		return []int{}
	}
	for i := 0; i < n; i++ {
		if len(deltas[i]) != d {
			outLog.Printf("Krum: ragged update %d (%d != %d)", i, len(deltas[i]), d)
			return []int{}
		}
	}
	m := n - f
	sel := make([]C.int64_t, m)
	var mOut C.int64_t
	var st C.int
	if bkGroup != nil {
		st = groupTopKRUM(deltas, n, d, f, sel, &mOut)
	} else {
		var pinner runtime.Pinner
		defer pinner.Unpin()
		var rowsC unsafe.Pointer
		rowsC = C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0))))
		defer C.free(rowsC)
		ptrs := unsafe.Slice((*unsafe.Pointer)(rowsC), n)
		for i := 0; i < n; i++ {
			pinner.Pin(&deltas[i][0])
			ptrs[i] = unsafe.Pointer(&deltas[i][0])
		}
		st = C.bk_multikrum_rows(bkCtx, (*unsafe.Pointer)(rowsC), C.BK_F64, C.int64_t(n),
			C.int64_t(d), C.int64_t(f), (*C.int64_t)(unsafe.Pointer(&sel[0])), &mOut, nil, nil)
	}
	if st != C.BK_OK {
		outLog.Printf("Krum failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return []int{}
	}
	logMargin()
	out := make([]int, int(mOut))
	for i := range out {
		out[i] = int(sel[i])
	}
	return out
}

// groupTopKRUM: BK_GPUS > 1 -- the rows packed into the C-owned pinned batch
// (serially, on this goroutine), then bk_group_multikrum, each GPU copying its
// column shard over its own PCIe link.
func groupTopKRUM(deltas [][]float64, n, d, f int, sel []C.int64_t, mOut *C.int64_t) C.int {
	need := int64(n) * int64(d) * 8
	if need > bkStageLen {
		if bkStage != nil {
			C.bk_stage_free(bkCtx, bkStage)
		}
		var p unsafe.Pointer
		if st := C.bk_stage_alloc(bkCtx, C.int64_t(need), &p); st != C.BK_OK {
			bkStage, bkStageLen = nil, 0
			return st
		}
		bkStage, bkStageLen = p, need
	}
	// pack [][]float64 rows into the pinned C buffer (row-major n x d)
	stage := unsafe.Slice((*float64)(bkStage), n*d)
	for i := 0; i < n; i++ {
		copy(stage[i*d:(i+1)*d], deltas[i])
	}
	return C.bk_group_multikrum(bkGroup, bkStage, C.BK_HOST_PINNED, C.BK_F64, C.int64_t(n),
		C.int64_t(d), C.int64_t(d), C.int64_t(f), (*C.int64_t)(unsafe.Pointer(&sel[0])), mOut,
		nil, nil)
}

// getTopKRUMIndexNoised is the same verifier call for updates that carry Delta
// and the averaged Noise vector separately (update.go:13-22; NoisedDelta =
// Delta + Noise at main.go:1524-1537): the noise is added on the GPU while the
// batch crosses PCIe (bk_multikrum_noised, SURVEY.md §8(f) row 3), so the
// verifier never builds NoisedDelta on the host.  k = 1 (Noise is already the
// mean over the noisers, main.go:1606-1653), which is bitwise Delta[i] +
// Noise[i]; updates without noise (-np=false) go with k = 0.  A batch that
// mixes the two falls back to getTopKRUMIndex over NoisedDelta.
func (krumval *KRUMValidator) getTopKRUMIndexNoised(updates []Update) []int {
	n := len(updates)
	if n == 0 || bkCtx == nil || bkGroup != nil {
		return krumval.getTopKRUMIndex(noisedDeltas(updates))
	}
	d := len(updates[0].Delta)
	k := 0
	if len(updates[0].Noise) > 0 {
		k = 1
	}
	for i := range updates {
		if len(updates[i].Delta) != d || len(updates[i].Noise) != k*d {
			return krumval.getTopKRUMIndex(noisedDeltas(updates))
		}
	}
	f := int(krumval.NumAdversaries * float64(n))
	if C.bk_check_args(C.int64_t(n), C.int64_t(d), C.int64_t(f)) != C.BK_OK {
		outLog.Printf("Krum: %s", C.GoString(C.bk_last_error()))
		return []int{}
	}
	need := int64(n) * int64(d) * 8 * int64(1+k)
	if need > bkStageLen {
		if bkStage != nil {
			C.bk_stage_free(bkCtx, bkStage)
		}
		var p unsafe.Pointer
		if C.bk_stage_alloc(bkCtx, C.int64_t(need), &p) != C.BK_OK {
			outLog.Printf("Krum: %s", C.GoString(C.bk_last_error()))
			bkStage, bkStageLen = nil, 0
			return []int{}
		}
		bkStage, bkStageLen = p, need
	}
	// pinned staging: Delta rows, then (k = 1) the Noise rows
	stage := unsafe.Slice((*float64)(bkStage), n*d*(1+k))
	for i := 0; i < n; i++ {
		copy(stage[i*d:(i+1)*d], updates[i].Delta)
		if k == 1 {
			copy(stage[(n+i)*d:(n+i+1)*d], updates[i].Noise)
		}
	}
	var noise *C.double
	if k == 1 {
		noise = (*C.double)(unsafe.Pointer(&stage[n*d]))
	}
	m := n - f
	sel := make([]C.int64_t, m)
	var mOut C.int64_t
	st := C.bk_multikrum_noised(bkCtx, (*C.double)(bkStage), C.int64_t(d), noise, C.int64_t(k),
		C.int64_t(d), C.BK_HOST_PINNED, C.int64_t(n), C.int64_t(d), C.int64_t(f),
		(*C.int64_t)(unsafe.Pointer(&sel[0])), &mOut, nil, nil, nil, 0)
	if st != C.BK_OK {
		outLog.Printf("Krum failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return []int{}
	}
	logMargin()
	out := make([]int, int(mOut))
	for i := range out {
		out[i] = int(sel[i])
	}
	return out
}

// logMargin reports a selection the reference could legitimately make
// differently (bk_selection_margin): the boundary gap between the highest
// selected and the lowest rejected score is within the rounding bound of the
// scores, or an exact tie (k = n-f-2 = 0 makes every score 0, as on the
// localTest.sh n = 4 verifier).  Otherwise numpy's argpartition over its own
// BLAS-rounded scores (logistic_validator.py:45,59-63) provably picks the same set.
func logMargin() {
	var gap, bound C.double
	var near C.int
	if C.bk_selection_margin(bkCtx, &gap, &bound, &near) == C.BK_OK && near != 0 {
		outLog.Printf("Krum: near tie at the selection boundary (gap %g <= bound %g); "+
			"ties resolved to the lower index", float64(gap), float64(bound))
	}
}

// ---- the miner's block, added to as the updates arrive (bk_block_*) ---------

// bkBlockDim is the length of the gradient the engine's block was begun with
// (0: no block); bkBlockLen counts the updates added to it.
var (
	bkBlockDim int
	bkBlockLen int
)

// beginBlockGPU starts the engine's block from bc.getLatestGradient(); call it
// where the miner resets blockUpdates for a new iteration.
func beginBlockGPU(globalW []float64) bool {
	d := len(globalW)
	bkBlockDim, bkBlockLen = 0, 0
	if bkCtx == nil || d == 0 {
		return false
	}
	var gp *C.double
	gp = (*C.double)(unsafe.Pointer(&globalW[0]))
	if st := C.bk_block_begin(bkCtx, C.BK_F64, C.int64_t(d), gp, C.BK_HOST, -1); st != C.BK_OK {
		outLog.Printf("bk_block_begin failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	bkBlockDim = d
	return true
}

// addBlockUpdateGPU replaces the append of addBlockUpdate (honest.go:330-334):
// the update's Delta goes to the GPU and is added to the running gradient at
// once if the update is accepted (a rejected update is counted and its Delta
// never read, honest.go:367-370).  Delta's backing array is pinned for the call
// and consumed on return.  Returns the number of updates in the block, -1 on an
// engine error (the caller then falls back to the host loop).
func addBlockUpdateGPU(update Update) int {
	if bkCtx == nil || bkBlockDim == 0 || len(update.Delta) != bkBlockDim {
		return -1
	}
	var pinner runtime.Pinner
	defer pinner.Unpin()
	var rowsC unsafe.Pointer
	rowsC = C.malloc(C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(rowsC)
	pinner.Pin(&update.Delta[0])
	unsafe.Slice((*unsafe.Pointer)(rowsC), 1)[0] = unsafe.Pointer(&update.Delta[0])
	var acc C.uint8_t
	if update.Accepted {
		acc = 1
	}
	if st := C.bk_block_add(bkCtx, (*unsafe.Pointer)(rowsC), &acc, 1, C.BK_HOST, nil); st != C.BK_OK {
		outLog.Printf("bk_block_add failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return -1
	}
	bkBlockLen++
	return bkBlockLen
}

// createBlockGPU replaces the update loop of createBlock (honest.go:346-388):
// the gradient with every accepted update added in arrival order, bit for bit
// what pulledGradientM.Add over blockUpdates gives.  The block is not consumed:
// the deadline path may call it, add late updates and call it again.  The
// stake bookkeeping stays in createBlock.  nil on an engine error.
func createBlockGPU() []float64 {
	if bkCtx == nil || bkBlockDim == 0 {
		return nil
	}
	out := make([]float64, bkBlockDim)
	var outp *C.double
	outp = (*C.double)(unsafe.Pointer(&out[0]))
	if st := C.bk_block_finish(bkCtx, outp, nil, nil); st != C.BK_OK {
		outLog.Printf("bk_block_finish failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil
	}
	return out
}

// The engine's evaluation-set slots (bk_eval_set_*): the set testModel scores
// and the attack set testAttackRate scores.
const (
	bkEvalTrainSet  = 0
	bkEvalAttackSet = 2
)

// setEvalLogisticGPU makes (X, y) the resident set `set`: X is nv x d, row-major
// (the creditcard train set that train_error reads).  Call it once at pyInit.
func setEvalLogisticGPU(set int, X []float64, y []float64, d int) bool {
	nv := len(y)
	if bkCtx == nil || nv == 0 || d == 0 || len(X) != nv*d {
		return false
	}
	var xp, yp *C.double
	xp = (*C.double)(unsafe.Pointer(&X[0]))
	yp = (*C.double)(unsafe.Pointer(&y[0]))
	if st := C.bk_eval_set_logistic(bkCtx, C.int(set), xp, C.int64_t(nv), C.int64_t(d), C.int64_t(d), yp); st != C.BK_OK {
		outLog.Printf("bk_eval_set_logistic failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	return true
}

// setEvalSoftmaxGPU is the torch datasets' form: X nv x dIn float32, y the
// labels in [0, classes) (the test set of getTestErr, the attack set of
// get17AttackRate).
func setEvalSoftmaxGPU(set int, X []float32, y []int32, dIn int, classes int) bool {
	nv := len(y)
	if bkCtx == nil || nv == 0 || dIn == 0 || len(X) != nv*dIn {
		return false
	}
	var xp *C.float
	var yp *C.int32_t
	xp = (*C.float)(unsafe.Pointer(&X[0]))
	yp = (*C.int32_t)(unsafe.Pointer(&y[0]))
	if st := C.bk_eval_set_softmax(bkCtx, C.int(set), xp, C.int64_t(nv), C.int64_t(dIn), C.int64_t(dIn), yp, C.int64_t(classes)); st != C.BK_OK {
		outLog.Printf("bk_eval_set_softmax failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	return true
}

func evalSetGPU(weights []float64, set int) float64 {
	d := len(weights)
	if bkCtx == nil || d == 0 {
		return -1
	}
	var wp *C.double
	wp = (*C.double)(unsafe.Pointer(&weights[0]))
	var setC C.int
	var errC C.double
	var wrongC C.int64_t
	setC = C.int(set)
	if st := C.bk_eval(bkCtx, wp, C.int64_t(d), C.BK_HOST, &setC, 1, &errC, &wrongC, nil); st != C.BK_OK {
		outLog.Printf("bk_eval failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return -1
	}
	return float64(errC)
}

// testModelGPU replaces testModel (honest.go:656-675): the model's error on the
// resident train / test set, what train_error / getTestErr return.  -1 on an
// engine error (the caller then falls back to the Python call).
func testModelGPU(weights []float64) float64 {
	return evalSetGPU(weights, bkEvalTrainSet)
}

// testAttackRateGPU replaces testAttackRate (honest.go:260-275).
func testAttackRateGPU(weights []float64) float64 {
	return evalSetGPU(weights, bkEvalAttackSet)
}

// createBlockEvalGPU is createBlockGPU with checkConvergence's scores of the
// new gradient (honest.go:141-162) from the same call: the model is scored
// where it is, on the device.  withAttack: the torch datasets' attack rate too
// (-1 otherwise).  nil on an engine error.
func createBlockEvalGPU(withAttack bool) ([]float64, float64, float64) {
	if bkCtx == nil || bkBlockDim == 0 {
		return nil, -1, -1
	}
	out := make([]float64, bkBlockDim)
	var outp *C.double
	outp = (*C.double)(unsafe.Pointer(&out[0]))
	setsC := make([]C.int, 2)
	errC := make([]C.double, 2)
	wrongC := make([]C.int64_t, 2)
	setsC[0], setsC[1] = bkEvalTrainSet, bkEvalAttackSet
	errC[1] = -1
	nsets := 1
	if withAttack {
		nsets = 2
	}
	if st := C.bk_block_finish_eval(bkCtx, outp, nil, nil, &setsC[0], C.int(nsets), &errC[0], &wrongC[0], nil); st != C.BK_OK {
		outLog.Printf("bk_block_finish_eval failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil, -1, -1
	}
	return out, float64(errC[0]), float64(errC[1])
}

// ---- secure aggregation: shares, their sum and recovery (bk_shares_*) -------
//
// The share values only: the G1 commitments and witnesses of fillPolynomialMap /
// createShareAndWitness are the bk_commit_* section's below; aggregateSecret's
// point sums stay in Go.

// bkSharesElems is the length of one part of the engine's store (chunks x the
// shares this miner holds; 0: no store).
var (
	bkSharesElems int
)

// generateSharesGPU replaces the evaluatedValue arithmetic of
// createSharesAndWitnesses for every chunk of deltaw (kyber.go:484-512,
// :579-646, as called by fillPolynomialMap for generateMinerSecretShares,
// kyber.go:456-482): y[chunk*totalShares+s] is the share at x = s - 10 of chunk
// `chunk`; miner m's Secrets are [held*m, held*(m+1)) of each chunk
// (extractMinerSecret, kyber.go:205-242).  nil on an engine error.
func generateSharesGPU(deltaw []float64, precision int, polySize int, totalShares int) []int64 {
	d := len(deltaw)
	if bkCtx == nil || d == 0 || polySize < 1 || totalShares < 1 {
		return nil
	}
	chunks := (d + polySize - 1) / polySize
	y := make([]int64, chunks*totalShares)
	var dp *C.double
	var yp *C.int64_t
	dp = (*C.double)(unsafe.Pointer(&deltaw[0]))
	yp = (*C.int64_t)(unsafe.Pointer(&y[0]))
	if st := C.bk_shares_generate(bkCtx, dp, C.BK_HOST, C.int64_t(d), C.int(precision), C.int(polySize), C.int(totalShares), yp); st != C.BK_OK {
		outLog.Printf("bk_shares_generate failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil
	}
	return y
}

// beginSharesGPU empties the engine's store for a new iteration; call it where
// the miner resets its secretList.  held: the shares of each chunk this miner
// holds, nCap: the most clients that can register.
func beginSharesGPU(d int, polySize int, held int, nCap int) bool {
	bkSharesElems = 0
	if bkCtx == nil || d == 0 || polySize < 1 {
		return false
	}
	if st := C.bk_shares_begin(bkCtx, C.int64_t(d), C.int(polySize), C.int(held), C.int64_t(nCap)); st != C.BK_OK {
		outLog.Printf("bk_shares_begin failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	bkSharesElems = (d + polySize - 1) / polySize * held
	return true
}

// addSecretShareGPU replaces the append of addSecretShare (honest.go:338-342,
// from Peer.RegisterSecret, main.go:256-286) for the share values: part is the
// client's Secrets' Y of every chunk, [chunk][share].  Returns the part's slot,
// which the caller keeps against the client's NodeID; -1 on an engine error.
func addSecretShareGPU(part []int64) int {
	if bkCtx == nil || bkSharesElems == 0 || len(part) != bkSharesElems {
		return -1
	}
	var pp *C.int64_t
	var slot C.int64_t
	pp = (*C.int64_t)(unsafe.Pointer(&part[0]))
	if st := C.bk_shares_add(bkCtx, pp, C.BK_HOST, &slot); st != C.BK_OK {
		outLog.Printf("bk_shares_add failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return -1
	}
	return int(slot)
}

// getMinerPartGPU replaces the Y sums of the aggregateSecret loop in
// getSecretShares (main.go:2157-2189, kyber.go:244-287; the reply of
// Peer.GetMinerPart, main.go:459-485): the wrapping int64 sum of the parts in
// `slots`, the slots of the agreed node list.  The sum also stays on the GPU as
// the engine's own aggregate.  nil on an engine error.
func getMinerPartGPU(slots []int64) []int64 {
	if bkCtx == nil || bkSharesElems == 0 || len(slots) == 0 {
		return nil
	}
	out := make([]int64, bkSharesElems)
	ns := len(slots)
	var sp, op *C.int64_t
	sp = (*C.int64_t)(unsafe.Pointer(&slots[0]))
	op = (*C.int64_t)(unsafe.Pointer(&out[0]))
	if st := C.bk_shares_sum(bkCtx, sp, C.int64_t(ns), op); st != C.BK_OK {
		outLog.Printf("bk_shares_sum failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil
	}
	return out
}

// recoverAggregateGPU replaces the recoverSecret loop of recoverAggregateUpdates
// (honest.go:442-502, kyber.go:809-857), updateIntToFloat and the model update of
// createBlockSecAgg (honest.go:408-409): parts[i] is miner i's aggregate
// ([chunk][share], held[i] shares per chunk; a nil entry, at most one: this
// miner's own, left on the GPU by getMinerPartGPU), xs the shares' X in part
// order.  Returns the new model, the aggregate delta and the number of chunks
// whose shares were inconsistent (their entries are 0); nil on an engine error.
func recoverAggregateGPU(globalW []float64, parts [][]int64, held []int, xs []int64, polySize int, precision int) ([]float64, []float64, int) {
	d := len(globalW)
	np := len(parts)
	if bkCtx == nil || d == 0 || np == 0 || len(held) != np || len(xs) == 0 {
		return nil, nil, -1
	}
	var pinner runtime.Pinner
	defer pinner.Unpin()
	var tableC unsafe.Pointer
	tableC = C.malloc(C.size_t(np) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(tableC)
	table := unsafe.Slice((*unsafe.Pointer)(tableC), np)
	heldC := make([]C.int, np)
	for i := range parts {
		heldC[i] = C.int(held[i])
		table[i] = nil
		if parts[i] != nil {
			pinner.Pin(&parts[i][0])
			table[i] = unsafe.Pointer(&parts[i][0])
		}
	}
	newW := make([]float64, d)
	delta := make([]float64, d)
	var wp, dp, gp *C.double
	var xp *C.int64_t
	var bad C.int64_t
	wp = (*C.double)(unsafe.Pointer(&globalW[0]))
	dp = (*C.double)(unsafe.Pointer(&delta[0]))
	gp = (*C.double)(unsafe.Pointer(&newW[0]))
	xp = (*C.int64_t)(unsafe.Pointer(&xs[0]))
	if st := C.sharesRecoverC(bkCtx, tableC, &heldC[0], xp, C.int(np), C.BK_HOST, C.int64_t(d), C.int(polySize), C.int(precision), wp, nil, dp, gp, &bad); st != C.BK_OK {
		outLog.Printf("bk_shares_recover failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil, nil, -1
	}
	return newW, delta, int(bad)
}

// ---- polynomial commitments in bn256 G1 (bk_commit_*) -----------------------
//
// The G1 side only: aggregateSecret's point sums, verifySecret's pairings and the
// Schnorr signatures stay in Go.  A point crosses as its MarshalBinary bytes.

// bkCommitKey is the number of key points resident in the engine (0: none).
var (
	bkCommitKey int
)

// pointFromBytesGPU is UnmarshalBinary of one 64-byte point (nil on an error).
func pointFromBytesGPU(buf []byte) kyber.Point {
	p := suite.G1().Point()
	if err := p.UnmarshalBinary(buf); err != nil {
		outLog.Printf("bn256 point from the engine does not unmarshal: %s", err)
		return nil
	}
	return p
}

// setCommitKeyGPU makes pkG1 the engine's resident key; call it once where the
// peer loads its PublicKey (extractKeys, before the first computeUpdate).
func setCommitKeyGPU(pkG1 []kyber.Point) bool {
	bkCommitKey = 0
	count := len(pkG1)
	if bkCtx == nil || count == 0 {
		return false
	}
	raw := make([]byte, 0, 64*count)
	for _, p := range pkG1 {
		b, err := p.MarshalBinary()
		if err != nil || len(b) != 64 {
			return false
		}
		raw = append(raw, b...)
	}
	var rp *C.uint8_t
	rp = (*C.uint8_t)(unsafe.Pointer(&raw[0]))
	if st := C.bk_commit_set_key(bkCtx, rp, C.int64_t(count)); st != C.BK_OK {
		outLog.Printf("bk_commit_set_key failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	bkCommitKey = count
	return true
}

// createCommitmentGPU replaces createCommitment(update, pkey.PKG1[first:first+len(update)])
// (kyber.go:533-562): computeUpdate's `createCommitment(deltasInt, pkey.PKG1)`
// (honest.go:186) becomes createCommitmentGPU(deltasInt, 0).  nil on an error.
func createCommitmentGPU(update []int64, first int) kyber.Point {
	n := len(update)
	if bkCtx == nil || n == 0 || first < 0 || first+n > bkCommitKey {
		return nil
	}
	out := make([]byte, 64)
	var up *C.int64_t
	var op *C.uint8_t
	up = (*C.int64_t)(unsafe.Pointer(&update[0]))
	op = (*C.uint8_t)(unsafe.Pointer(&out[0]))
	if st := C.bk_commit_msm(bkCtx, up, C.BK_HOST, C.int64_t(n), C.int64_t(first), op); st != C.BK_OK {
		outLog.Printf("bk_commit_msm failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil
	}
	return pointFromBytesGPU(out)
}

// verifyCommitmentGPU replaces verifyCommitment (kyber.go:564-577) over
// pkey.PKG1[first:first+len(update)].
func verifyCommitmentGPU(update []int64, first int, committedUpdate kyber.Point) bool {
	n := len(update)
	if bkCtx == nil || n == 0 || first < 0 || first+n > bkCommitKey {
		return false
	}
	want, err := committedUpdate.MarshalBinary()
	if err != nil || len(want) != 64 {
		return false
	}
	var up *C.int64_t
	var wp *C.uint8_t
	var ok C.int
	up = (*C.int64_t)(unsafe.Pointer(&update[0]))
	wp = (*C.uint8_t)(unsafe.Pointer(&want[0]))
	if st := C.bk_commit_verify(bkCtx, up, C.BK_HOST, C.int64_t(n), C.int64_t(first), wp, &ok); st != C.BK_OK {
		outLog.Printf("bk_commit_verify failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return false
	}
	return ok == 1
}

// fillPolynomialMapGPU replaces the G1 arithmetic of generateMinerSecretShares
// (kyber.go:456-482): its CommitmentUpdate (the first result), and for
// fillPolynomialMap (kyber.go:172-202) each chunk's Commitment (the second,
// [chunk]) and Witnesses (the third, [chunk][share]; createShareAndWitness,
// kyber.go:579-646).  The Secrets come from generateSharesGPU.  nil on an error.
func fillPolynomialMapGPU(deltaw []float64, precision int, polySize int, totalShares int) (kyber.Point, []kyber.Point, [][]kyber.Point) {
	d := len(deltaw)
	if bkCtx == nil || d == 0 || d > bkCommitKey || polySize < 1 || totalShares < 1 {
		return nil, nil, nil
	}
	chunks := (d + polySize - 1) / polySize
	whole := make([]byte, 64)
	chunkRaw := make([]byte, 64*chunks)
	witRaw := make([]byte, 64*chunks*totalShares)
	var dp *C.double
	var cp, kp, wp *C.uint8_t
	dp = (*C.double)(unsafe.Pointer(&deltaw[0]))
	cp = (*C.uint8_t)(unsafe.Pointer(&whole[0]))
	kp = (*C.uint8_t)(unsafe.Pointer(&chunkRaw[0]))
	wp = (*C.uint8_t)(unsafe.Pointer(&witRaw[0]))
	if st := C.bk_commit_generate(bkCtx, dp, nil, C.BK_HOST, C.int64_t(d), C.int(precision), C.int(polySize), C.int(totalShares), cp, kp, wp); st != C.BK_OK {
		outLog.Printf("bk_commit_generate failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil, nil, nil
	}
	commitment := pointFromBytesGPU(whole)
	if commitment == nil {
		return nil, nil, nil
	}
	chunkPoints := make([]kyber.Point, chunks)
	witnesses := make([][]kyber.Point, chunks)
	for c := 0; c < chunks; c++ {
		if chunkPoints[c] = pointFromBytesGPU(chunkRaw[64*c : 64*c+64]); chunkPoints[c] == nil {
			return nil, nil, nil
		}
		witnesses[c] = make([]kyber.Point, totalShares)
		for s := 0; s < totalShares; s++ {
			o := 64 * (c*totalShares + s)
			if witnesses[c][s] = pointFromBytesGPU(witRaw[o : o+64]); witnesses[c][s] == nil {
				return nil, nil, nil
			}
		}
	}
	return commitment, chunkPoints, witnesses
}

// ---- the gradient step on the peer's resident shard (bk_grad_*) -------------

// The shard's model length (0: no shard), its kind and the step's constants
// (logistic_model.py's alpha and lammy, client.py's clip_grad_norm bound).
// bkGradNoise, when non-nil, is getNoise(iteration) as the caller computed it
// for the next step (d entries); the engine adds it to the delta.
var (
	bkGradDim       int
	bkGradSoftmax   bool
	bkGradBatch     int
	bkGradPrecision int
	bkGradAlpha     float64 = 1e-2
	bkGradLammy     float64 = 0.01
	bkGradMaxNorm   float64 = 100.0
	bkGradNoise     []float64
)

// initGradGPU makes the peer's training shard resident; call it once at pyInit.
// classes == 0: the logistic model, X nn x d row-major with labels y.  Else the
// torch softmax model, X32 nn x d float32 with labels y32 in [0, classes).
// batchSize is the reference's this_batch_size (the logistic divisor),
// precision the commitment's (updateFloatToInt).
func initGradGPU(X []float64, y []float64, X32 []float32, y32 []int32, d int, classes int, batchSize int, precision int) bool {
	bkGradDim = 0
	if bkCtx == nil || d == 0 || batchSize < 1 {
		return false
	}
	if classes == 0 {
		nn := len(y)
		if nn == 0 || len(X) != nn*d {
			return false
		}
		var xp, yp *C.double
		xp = (*C.double)(unsafe.Pointer(&X[0]))
		yp = (*C.double)(unsafe.Pointer(&y[0]))
		if st := C.bk_grad_set_logistic(bkCtx, xp, C.int64_t(nn), C.int64_t(d), C.int64_t(d), yp); st != C.BK_OK {
			outLog.Printf("bk_grad_set_logistic failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
			return false
		}
		bkGradDim = d
	} else {
		nn := len(y32)
		if nn == 0 || len(X32) != nn*d {
			return false
		}
		var xfp *C.float
		var yip *C.int32_t
		xfp = (*C.float)(unsafe.Pointer(&X32[0]))
		yip = (*C.int32_t)(unsafe.Pointer(&y32[0]))
		if st := C.bk_grad_set_softmax(bkCtx, xfp, C.int64_t(nn), C.int64_t(d), C.int64_t(d), yip, C.int64_t(classes)); st != C.BK_OK {
			outLog.Printf("bk_grad_set_softmax failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
			return false
		}
		bkGradDim = classes * (d + 1)
	}
	bkGradSoftmax = classes != 0
	bkGradBatch = batchSize
	bkGradPrecision = precision
	return true
}

// oneGradientStepGPU replaces oneGradientStep and the updateFloatToInt behind it
// in computeUpdate (honest.go:165-200, 284-324): the delta of the model globalW
// on the rows idx of the shard (the mini-batch the caller drew; nil: every row)
// and its quantisation.  nil, nil on an engine error.
func oneGradientStepGPU(globalW []float64, idx []int64) ([]float64, []int64) {
	d := len(globalW)
	if bkCtx == nil || d == 0 || d != bkGradDim {
		return nil, nil
	}
	delta := make([]float64, d)
	q := make([]int64, d)
	var wp, dp, np *C.double
	var qp, ip *C.int64_t
	wp = (*C.double)(unsafe.Pointer(&globalW[0]))
	dp = (*C.double)(unsafe.Pointer(&delta[0]))
	qp = (*C.int64_t)(unsafe.Pointer(&q[0]))
	if len(bkGradNoise) == d {
		np = (*C.double)(unsafe.Pointer(&bkGradNoise[0]))
	}
	count := len(idx)
	if count > 0 {
		ip = (*C.int64_t)(unsafe.Pointer(&idx[0]))
	}
	var st C.int
	if bkGradSoftmax {
		st = C.bk_grad_softmax(bkCtx, wp, C.BK_HOST, ip, C.int64_t(count), C.double(bkGradMaxNorm), np, C.int(bkGradPrecision), dp, qp, nil, nil)
	} else {
		st = C.bk_grad_logistic(bkCtx, wp, C.BK_HOST, ip, C.int64_t(count), C.int64_t(bkGradBatch), C.double(bkGradAlpha), C.double(bkGradLammy), np, C.int(bkGradPrecision), dp, qp, nil)
	}
	if st != C.BK_OK {
		outLog.Printf("bk_grad failed (%d): %s", int(st), C.GoString(C.bk_last_error()))
		return nil, nil
	}
	return delta, q
}

func noisedDeltas(updates []Update) [][]float64 {
	deltas := make([][]float64, len(updates))
	for i := range updates {
		deltas[i] = updates[i].NoisedDelta
	}
	return deltas
}
