// integration/KeyFrameDatabase_hip.cc -- src/KeyFrameDatabase.cc (whole file) over the device store of orbm_kfdb_*: the BowVector of
// every added keyframe lives in HBM under a slot, and each Detect method is ONE library call (orbm_kfdb_query: per slot the number
// of shared words, the query index of the first shared word, the float L1 score) followed by the host half of the query,
// orbslam_hip::KfdbCandidatesFromCounts (include/orbslam_hip.hpp), run over KeyFrame* and the reference's own KeyFrame fields
// (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore).  This file holds the KeyFrame* <-> slot table and
// the adaptors, no logic of its own.  mvInvertedFile stays empty.
//   KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates    src/KeyFrameDatabase.cc:40-309
//   HipDetectLoopMinScore        LoopClosing::DetectLoop's minScore loop    src/LoopClosing.cc:124-138    one orbm_kfdb_score
//   HipKeyFrameDatabaseRelease   frees the device store of a database that is about to be deleted
// include/KeyFrameDatabase.h is not edited (reference.patch is pinned), so the table of a database lives here, keyed by the database;
// the header declares no destructor, hence HipKeyFrameDatabaseRelease (a database constructed at the address of one that was never
// released starts from an empty table all the same).  A call the library refuses is reported on std::cerr with the library's
// reason and changes nothing: add then leaves the keyframe out of the database, a Detect method returns no candidates.
// Like the other shells this file cannot be compiled where OpenCV / DBoW2 are absent.
#include "KeyFrameDatabase.h"

#include <algorithm>
#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "orbslam_hip.hpp"

using namespace std;

namespace ORB_SLAM2
{

namespace
{
struct HipDatabase {
    orbm_kfdb *db = NULL;
    mutex mu;                           // guards the two tables (instead of KeyFrameDatabase::mMutex, which a free function cannot take)
    vector<KeyFrame*> kfOfSlot;         // NULL: erased
    map<KeyFrame*, int> slotOf;
};
mutex gTablesMutex;
map<const KeyFrameDatabase*, HipDatabase> gTables;

HipDatabase &TableOf(const KeyFrameDatabase *pDB)
{
    unique_lock<mutex> lock(gTablesMutex);
    return gTables[pDB];
}

bool Refused(int rc, const char *what)
{
    if (rc == ORBX_OK) return false;
    cerr << "KeyFrameDatabase_hip: " << what << ": " << orbx_last_error() << endl;
    return true;
}

// DBoW2::BowVector (std::map<WordId, WordValue>) in map order
struct FlatBowVec {
    vector<int32_t> words;
    vector<double> values;
    explicit FlatBowVec(const DBoW2::BowVector &v)
    {
        for (DBoW2::BowVector::const_iterator vit = v.begin(), vend = v.end(); vit != vend; vit++) {
            words.push_back((int32_t)vit->first);
            values.push_back(vit->second);
        }
    }
};

// One query: what orbm_kfdb_query leaves per slot.  false: the library refused (orbx_last_error() has the reason).
struct Counts {
    vector<int32_t> common, first;
    vector<float> score;
};
bool QueryCounts(HipDatabase &t, const DBoW2::BowVector &bow, Counts &c)
{
    const FlatBowVec q(bow);
    const size_t n = t.kfOfSlot.size() ? t.kfOfSlot.size() : 1;
    c.common.assign(n, 0); c.first.assign(n, -1); c.score.assign(n, 0.0f);
    return !Refused(orbm_kfdb_query(t.db, q.words.data(), q.values.data(), (int)q.words.size(), c.common.data(), c.first.data(), c.score.data()), "query");
}

void BestCovisibles(KeyFrame *pKF, vector<KeyFrame*> &out) { out = pKF->GetBestCovisibilityKeyFrames(10); }
}

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc):
    mpVoc(&voc)
{
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    if (t.db) orbm_kfdb_destroy(t.db);               // the table of a database that lived at this address and was never released
    t.db = NULL;
    t.kfOfSlot.clear();
    t.slotOf.clear();
    Refused(orbm_kfdb_create((int)voc.size(), &t.db), "create");
}

void HipKeyFrameDatabaseRelease(KeyFrameDatabase *pDB)
{
    unique_lock<mutex> lock(gTablesMutex);
    map<const KeyFrameDatabase*, HipDatabase>::iterator it = gTables.find(pDB);
    if (it == gTables.end())
        return;
    if (it->second.db) orbm_kfdb_destroy(it->second.db);
    gTables.erase(it);
}

void KeyFrameDatabase::add(KeyFrame *pKF)
{
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    const FlatBowVec row(pKF->mBowVec);
    int32_t slot = -1;
    if (Refused(orbm_kfdb_add(t.db, row.words.data(), row.values.data(), (int)row.words.size(), &slot), "add"))
        return;
    t.kfOfSlot.resize(slot + 1, static_cast<KeyFrame*>(NULL));
    t.kfOfSlot[slot] = pKF;
    t.slotOf[pKF] = slot;
}

void KeyFrameDatabase::erase(KeyFrame* pKF)
{
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    map<KeyFrame*, int>::iterator it = t.slotOf.find(pKF);
    if (it == t.slotOf.end())
        return;                                      // never added (the reference's loop finds nothing either)
    if (Refused(orbm_kfdb_erase(t.db, it->second), "erase"))
        return;
    t.kfOfSlot[it->second] = NULL;
    t.slotOf.erase(it);
}

void KeyFrameDatabase::clear()
{
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    if (Refused(orbm_kfdb_clear(t.db), "clear"))
        return;
    t.kfOfSlot.clear();
    t.slotOf.clear();
}

// The list of keyframes sharing words, the connected keyframes, the word cut, minScore and the covisibility fold are
// orbslam_hip::KfdbCandidatesFromCounts (include/orbslam_hip.hpp: the one statement of that logic, which the library's tests run
// through orbslam_hip::KeyFrameDatabase), here over KeyFrame* and the reference's own fields.
vector<KeyFrame*> KeyFrameDatabase::DetectLoopCandidates(KeyFrame* pKF, float minScore)
{
    const set<KeyFrame*> spConnected = pKF->GetConnectedKeyFrames();
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    Counts c;
    if (!QueryCounts(t, pKF->mBowVec, c))
        return vector<KeyFrame*>();
    return orbslam_hip::KfdbCandidatesFromCounts<KeyFrame*>(
        true, c.common.data(), c.first.data(), c.score.data(), t.kfOfSlot.size(), pKF->mnId, minScore,
        [&t](int slot) { return t.kfOfSlot[slot]; },
        [](KeyFrame *k) { return orbslam_hip::KfdbQueryFields{k->mnLoopQuery, k->mnLoopWords, k->mLoopScore}; },
        [&spConnected](KeyFrame *k) { return spConnected.count(k) != 0; }, BestCovisibles);
}

vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F)
{
    HipDatabase &t = TableOf(this);
    unique_lock<mutex> lock(t.mu);
    Counts c;
    if (!QueryCounts(t, F->mBowVec, c))
        return vector<KeyFrame*>();
    return orbslam_hip::KfdbCandidatesFromCounts<KeyFrame*>(
        false, c.common.data(), c.first.data(), c.score.data(), t.kfOfSlot.size(), F->mnId, 0.0f,
        [&t](int slot) { return t.kfOfSlot[slot]; },
        [](KeyFrame *k) { return orbslam_hip::KfdbQueryFields{k->mnRelocQuery, k->mnRelocWords, k->mRelocScore}; },
        [](KeyFrame *) { return false; }, BestCovisibles);
}

// LoopClosing::DetectLoop's minScore loop (src/LoopClosing.cc:124-138): `float minScore; if (!HipDetectLoopMinScore(mpKeyFrameDB,
// mpORBVocabulary, mpCurrentKF, minScore)) { ...as when there is no candidate... }`.  Every connected keyframe that is in the
// database is scored in one library call.  A connected keyframe that is not (it still waits in the loop queue, so its row is not
// resident) keeps the reference's own call.  false: the library refused and minScore is not to be used.
bool HipDetectLoopMinScore(KeyFrameDatabase *pDB, const ORBVocabulary *pVoc, KeyFrame *pCurrentKF, float &minScore)
{
    const vector<KeyFrame*> vpConnected = pCurrentKF->GetVectorCovisibleKeyFrames();
    const DBoW2::BowVector &bowCurrent = pCurrentKF->mBowVec;
    minScore = 1;
    HipDatabase &t = TableOf(pDB);
    unique_lock<mutex> lock(t.mu);
    vector<int32_t> slots;
    for (size_t i = 0; i < vpConnected.size(); i++) {
        KeyFrame* pKF = vpConnected[i];
        if (pKF->isBad())
            continue;
        map<KeyFrame*, int>::iterator it = t.slotOf.find(pKF);
        if (it != t.slotOf.end())
            slots.push_back(it->second);
        else
            minScore = min(minScore, (float)pVoc->score(bowCurrent, pKF->mBowVec));
    }
    if (slots.empty())
        return true;
    const FlatBowVec q(bowCurrent);
    vector<float> score(slots.size());
    if (Refused(orbm_kfdb_score(t.db, q.words.data(), q.values.data(), (int)q.words.size(), slots.data(), (int)slots.size(), score.data()), "score"))
        return false;
    for (size_t i = 0; i < score.size(); i++)
        minScore = min(minScore, score[i]);
    return true;
}

} //namespace ORB_SLAM
