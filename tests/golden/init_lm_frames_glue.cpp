// Glue for tests/golden/make_init_lm_frames_golden.py: runs the REFERENCE'S OWN CoarseInitializer::trackFrame (compiled into oracle/_ref/libref.so by oracle/Makefile.ref)
// on levels given as flat arrays and frames given as images.  Nothing of the reference is restated here: the glue fills the members trackFrame reads (the points setFirst
// would make, firstFrame, fixAffine), calls the member, and reads members back.
#include <algorithm>
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
#include "util/FrameShell.h"
#include "FullSystem/HessianBlocks.h"
#include "FullSystem/CoarseInitializer.h"
#undef private
#undef protected

using namespace dso;

struct Glue {
	CoarseInitializer* ci;
	CalibHessian* calib;
	std::vector<FrameHessian*> frames;
};

static FrameHessian* makeFrame(Glue* g, const float* img, int id)
{
	FrameHessian* fh = new FrameHessian();
	FrameShell* shell = new FrameShell();
	shell->camToWorld = SE3();
	shell->aff_g2l = AffLight(0, 0);
	shell->marginalizedAt = shell->id = id;
	shell->timestamp = id;
	shell->incoming_id = id;
	fh->shell = shell;
	fh->ab_exposure = 0;   // (no exposure: trackFrame keeps thisToNext_aff as the start of aff, :121-122)
	std::vector<float> copy(img, img + wG[0] * hG[0]);
	fh->makeImages(copy.data(), g->calib);
	g->frames.push_back(fh);
	return fh;
}

extern "C" {

void* ilf_create(int w, int h, const float* K4, const float* first_img, int fixAffine, int* levels)
{
	Eigen::Matrix3f K = Eigen::Matrix3f::Identity();
	K(0, 0) = K4[0]; K(1, 1) = K4[1]; K(0, 2) = K4[2]; K(1, 2) = K4[3];
	setGlobalCalib(w, h, K);
	multiThreading = false;
	setting_weightZeroPriorDSOInitY = 0; setting_weightZeroPriorDSOInitX = 0;
	Glue* g = new Glue();
	g->calib = new CalibHessian();
	VecC kv; kv << K4[0], K4[1], K4[2], K4[3];
	g->calib->setValueScaled(kv);
	g->ci = new CoarseInitializer(w, h);
	g->ci->makeK(g->calib);
	g->ci->firstFrame = makeFrame(g, first_img, 0);
	g->ci->fixAffine = fixAffine != 0;
	g->ci->printDebug = false;
	g->ci->snapped = false;
	g->ci->frameID = g->ci->snappedAt = 0;
	g->ci->thisToNext = SE3();
	g->ci->thisToNext_aff = AffLight(0, 0);
	*levels = pyrLevelsUsed;
	return g;
}
void ilf_destroy(void* p)
{
	Glue* g = (Glue*)p;
	g->ci->firstFrame = 0; g->ci->newFrame = 0;
	delete g->ci;
	for (FrameHessian* fh : g->frames) { fh->efFrame = 0; FrameShell* s = fh->shell; delete fh; delete s; }
	delete g->calib;
	delete g;
}
// the intrinsics of a level and their inverse as the initializer holds them
void ilf_get_k(void* p, int lvl, float* K4, double* Ki9)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	K4[0] = ci->fx[lvl]; K4[1] = ci->fy[lvl]; K4[2] = ci->cx[lvl]; K4[3] = ci->cy[lvl];
	for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Ki9[r * 3 + c] = ci->Ki[lvl](r, c);
}
void ilf_get_wm(void* p, float* wM8) { for (int i = 0; i < 8; i++) wM8[i] = ((Glue*)p)->ci->wM.diagonal()[i]; }
// the level's points from flat arrays, as setFirst and makeNN would leave them
void ilf_set_level(void* p, int lvl, int n, const float* u, const float* v, const float* outlierTH, const int* neighbours10, const int* parent)
{
	CoarseInitializer* ci = ((Glue*)p)->ci;
	if (ci->points[lvl] != 0) delete[] ci->points[lvl];
	ci->points[lvl] = new Pnt[n > 0 ? n : 1];
	ci->numPoints[lvl] = n;
	for (int i = 0; i < n; i++)
	{
		Pnt& q = ci->points[lvl][i];
		memset((void*)&q, 0, sizeof(Pnt));
		q.u = u[i]; q.v = v[i]; q.idepth = 1; q.iR = 1; q.isGood = true; q.energy.setZero(); q.lastHessian = 0; q.lastHessian_new = 0; q.my_type = 1;
		q.idepth_new = 1; q.outlierTH = outlierTH[i];
		for (int k = 0; k < 10; k++) q.neighbours[k] = neighbours10[10 * i + k];
		q.parent = parent ? parent[i] : -1;
	}
}
void ilf_get_level(void* p, int lvl, float* idepth, float* iR, unsigned char* isGood, float* energy2, float* lastHessian, float* idepth_new, unsigned char* isGood_new,
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
// CoarseInitializer::trackFrame on a new image; state10: thisToNext (t, then the quaternion x y z w), thisToNext_aff (a, b), snapped
void ilf_track_frame(void* p, const float* img, int id, double* state10)
{
	Glue* g = (Glue*)p;
	FrameHessian* fh = makeFrame(g, img, id);
	std::vector<IOWrap::Output3DWrapper*> wraps;
	g->ci->trackFrame(fh, wraps);
	const SE3& T = g->ci->thisToNext;
	state10[0] = T.translation()[0]; state10[1] = T.translation()[1]; state10[2] = T.translation()[2];
	const Eigen::Quaterniond& q = T.unit_quaternion();
	state10[3] = q.x(); state10[4] = q.y(); state10[5] = q.z(); state10[6] = q.w();
	state10[7] = g->ci->thisToNext_aff.a; state10[8] = g->ci->thisToNext_aff.b; state10[9] = g->ci->snapped ? 1 : 0;
}

}  // extern "C"
