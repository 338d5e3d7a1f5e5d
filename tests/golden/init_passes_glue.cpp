// Glue for tests/golden/make_init_passes_golden.py: runs the REFERENCE'S OWN per-point members of CoarseInitializer (compiled into oracle/_ref/libref.so by
// oracle/Makefile.ref) — resetPoints, doStep, applyStep, optReg, calcEC, propagateUp, propagateDown — on levels given as flat arrays.  Nothing of the reference is restated
// here but the three assignments of trackFrame's reset for a frame that has not snapped (CoarseInitializer.cpp:100-114), which are not a member of their own.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include "util/NumType.h"
#include "util/settings.h"
#include "util/globalCalib.h"
#include "FullSystem/HessianBlocks.h"
#include "FullSystem/CoarseInitializer.h"
#undef private
#undef protected

using namespace dso;

struct Glue {
	CoarseInitializer* ci;
	int w, h;
};

extern "C" {

// -> the handle; *levels = pyrLevelsUsed of a w x h image (resetPoints takes its second branch on level pyrLevelsUsed - 1 only)
void* ipg_create(int w, int h, int* levels)
{
	Eigen::Matrix3f K = Eigen::Matrix3f::Identity();
	K(0, 0) = K(1, 1) = (float)w; K(0, 2) = w * 0.5f; K(1, 2) = h * 0.5f;
	setGlobalCalib(w, h, K);
	Glue* g = new Glue();
	g->ci = new CoarseInitializer(w, h);
	g->w = w; g->h = h;
	g->ci->regWeight = 0.8f; g->ci->couplingWeight = 1.0f; g->ci->snapped = false;
	*levels = pyrLevelsUsed;
	return g;
}
void ipg_destroy(void* p) { Glue* g = (Glue*)p; delete g->ci; delete g; }
void ipg_settings(void* p, float regWeight, float couplingWeight, int snapped)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	ci->regWeight = regWeight; ci->couplingWeight = couplingWeight; ci->snapped = snapped != 0;
}

// the level's points from flat arrays; the two JbBuffers are the initializer's, shared by all levels as in the reference
void ipg_set_level(void* p, int lvl, int n, const float* u, const float* v, const float* idepth, const float* iR, const unsigned char* isGood, const float* energy2,
                   const float* outlierTH, const float* lastHessian, const float* idepth_new, const unsigned char* isGood_new, const float* energy_new2,
                   const float* lastHessian_new, const float* maxstep, const int* neighbours10, const int* parent)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	if (ci->points[lvl] != 0) delete[] ci->points[lvl];
	ci->points[lvl] = new Pnt[n > 0 ? n : 1];
	ci->numPoints[lvl] = n;
	for (int i = 0; i < n; i++)
	{
		Pnt& q = ci->points[lvl][i];
		memset((void*)&q, 0, sizeof(Pnt));
		q.u = u[i]; q.v = v[i]; q.idepth = idepth[i]; q.iR = iR[i]; q.isGood = isGood[i] != 0;
		q.energy = Vec2f(energy2[2 * i], energy2[2 * i + 1]); q.outlierTH = outlierTH[i]; q.lastHessian = lastHessian[i];
		q.idepth_new = idepth_new[i]; q.isGood_new = isGood_new[i] != 0; q.energy_new = Vec2f(energy_new2[2 * i], energy_new2[2 * i + 1]);
		q.lastHessian_new = lastHessian_new[i]; q.maxstep = maxstep[i];
		for (int k = 0; k < 10; k++) q.neighbours[k] = neighbours10[10 * i + k];
		q.parent = parent ? parent[i] : -1;
	}
}
void ipg_get_level(void* p, int lvl, float* idepth, float* iR, unsigned char* isGood, float* energy2, float* lastHessian, float* idepth_new, unsigned char* isGood_new,
                   float* energy_new2, float* lastHessian_new, float* maxstep)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	for (int i = 0; i < ci->numPoints[lvl]; i++)
	{
		const Pnt& q = ci->points[lvl][i];
		idepth[i] = q.idepth; iR[i] = q.iR; isGood[i] = q.isGood ? 1 : 0; energy2[2 * i] = q.energy[0]; energy2[2 * i + 1] = q.energy[1]; lastHessian[i] = q.lastHessian;
		idepth_new[i] = q.idepth_new; isGood_new[i] = q.isGood_new ? 1 : 0; energy_new2[2 * i] = q.energy_new[0]; energy_new2[2 * i + 1] = q.energy_new[1];
		lastHessian_new[i] = q.lastHessian_new; maxstep[i] = q.maxstep;
	}
}
void ipg_set_jb(void* p, int n, const float* jb10, const float* jb_new10)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	for (int i = 0; i < n; i++) for (int k = 0; k < 10; k++) { ci->JbBuffer[i][k] = jb10[10 * i + k]; ci->JbBuffer_new[i][k] = jb_new10[10 * i + k]; }
}
void ipg_get_jb(void* p, int n, float* jb10, float* jb_new10)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	for (int i = 0; i < n; i++) for (int k = 0; k < 10; k++) { jb10[10 * i + k] = ci->JbBuffer[i][k]; jb_new10[10 * i + k] = ci->JbBuffer_new[i][k]; }
}

void ipg_reset_points(void* p, int lvl) { ((Glue*)p)->ci->resetPoints(lvl); }
void ipg_do_step(void* p, int lvl, float lambda, const float* inc8)
{
	Vec8f inc;
	for (int k = 0; k < 8; k++) inc[k] = inc8[k];
	((Glue*)p)->ci->doStep(lvl, lambda, inc);
}
void ipg_apply_step(void* p, int lvl) { ((Glue*)p)->ci->applyStep(lvl); }
void ipg_opt_reg(void* p, int lvl) { ((Glue*)p)->ci->optReg(lvl); }
void ipg_calc_ec(void* p, int lvl, float* out3)
{
	Vec3f r = ((Glue*)p)->ci->calcEC(lvl);
	out3[0] = r[0]; out3[1] = r[1]; out3[2] = r[2];
}
void ipg_propagate_up(void* p, int srcLvl) { ((Glue*)p)->ci->propagateUp(srcLvl); }
void ipg_propagate_down(void* p, int srcLvl) { ((Glue*)p)->ci->propagateDown(srcLvl); }
// CoarseInitializer.cpp:100-114 for one level (the loop body there, verbatim in effect: three assignments per point)
void ipg_reset_unsnapped(void* p, int lvl)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	for (int i = 0; i < ci->numPoints[lvl]; i++) { ci->points[lvl][i].iR = 1; ci->points[lvl][i].idepth_new = 1; ci->points[lvl][i].lastHessian = 0; }
}

// median wall time in microseconds of `reps` calls of one member on level lvl: 0 doStep, 1 applyStep, 2 optReg, 3 calcEC, 4 resetPoints
double ipg_time(void* p, int lvl, int what, int reps)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	Vec8f inc; for (int k = 0; k < 8; k++) inc[k] = 1e-3f * (k + 1);
	std::vector<double> t;
	volatile float sink = 0;
	for (int r = 0; r < reps; r++)
	{
		auto t0 = std::chrono::steady_clock::now();
		if (what == 0) ci->doStep(lvl, 0.1f, inc);
		else if (what == 1) ci->applyStep(lvl);
		else if (what == 2) ci->optReg(lvl);
		else if (what == 3) sink = sink + ci->calcEC(lvl)[0];
		else ci->resetPoints(lvl);
		auto t1 = std::chrono::steady_clock::now();
		t.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
	}
	std::sort(t.begin(), t.end());
	return t[t.size() / 2];
}

}  // extern "C"
