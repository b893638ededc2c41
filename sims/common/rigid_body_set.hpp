// What the managers of the rigid-body simulators share, on both backends: the
// convex hulls they are made of (no file importers here: shapes are generated,
// instances scale them) and the recipe that bakes them into an ObjectManager.
//
// Vertex order, face order and winding of a hull decide the baked half-edge
// mesh and the mass properties, and hull indices are baked into the assets: a
// simulator's results change with either.
//
// The calls are the reference's API, spelled the way a reference simulator's
// manager spells them (PhysicsLoader, RigidBodyAssets::processRigidBodyAssets,
// loadRigidBodies): like mgr_impl.inl this file doubles as the "links
// unchanged" check of the header overlay.
#pragma once

#include "sim_c_api.h"

#include <madrona/physics_loader.hpp>
#include <madrona/physics_assets.hpp>
#include <madrona/importer.hpp>
#include <madrona/stack_alloc.hpp>

#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <vector>

namespace simmgr {

// A convex hull as polygons (outward CCW), owning its arrays.
struct HullSource {
    std::vector<madrona::math::Vector3> positions;
    std::vector<uint32_t> indices;
    std::vector<uint32_t> faceCounts;

    madrona::imp::SourceMesh mesh()
    {
        madrona::imp::SourceMesh m {};
        m.positions = positions.data();
        m.indices = indices.data();
        m.faceCounts = faceCounts.data();
        m.numVertices = (uint32_t)positions.size();
        m.numFaces = (uint32_t)faceCounts.size();
        return m;
    }

    // An axis-aligned box [lo, hi].
    static HullSource box(madrona::math::Vector3 lo, madrona::math::Vector3 hi)
    {
        return HullSource {
            {
                { lo.x, lo.y, lo.z }, { hi.x, lo.y, lo.z },
                { hi.x, hi.y, lo.z }, { lo.x, hi.y, lo.z },
                { lo.x, lo.y, hi.z }, { hi.x, lo.y, hi.z },
                { hi.x, hi.y, hi.z }, { lo.x, hi.y, hi.z },
            },
            {
                0, 3, 2, 1,     // -z
                4, 5, 6, 7,     // +z
                0, 1, 5, 4,     // -y
                2, 3, 7, 6,     // +y
                0, 4, 7, 3,     // -x
                1, 2, 6, 5,     // +x
            },
            { 4, 4, 4, 4, 4, 4 },
        };
    }

    // The cube [lo, hi]^3; the unit cube is box(-0.5f, 0.5f).
    static HullSource box(float lo, float hi)
    {
        return box({ lo, lo, lo }, { hi, hi, hi });
    }

    // The unit wedge (right-triangle cross-section: the slope rises from
    // y = -0.5 to y = +0.5; 6 vertices, 3 quads + 2 triangles).
    static HullSource wedge()
    {
        return HullSource {
            {
                { -0.5f, -0.5f, -0.5f }, { 0.5f, -0.5f, -0.5f },
                { 0.5f, 0.5f, -0.5f }, { -0.5f, 0.5f, -0.5f },
                { -0.5f, 0.5f, 0.5f }, { 0.5f, 0.5f, 0.5f },
            },
            {
                0, 3, 2, 1,     // -z
                2, 3, 4, 5,     // +y
                0, 1, 5, 4,     // slope (-y, +z)
                0, 4, 3,        // -x
                1, 2, 5,        // +x
            },
            { 4, 4, 4, 3, 3 },
        };
    }

    // A regular n-gon prism ("coin") of radius r and height h, axis along z.
    static HullSource prism(uint32_t n, float r, float h)
    {
        HullSource m;
        for (uint32_t ring = 0; ring < 2; ring++) {
            for (uint32_t i = 0; i < n; i++) {
                float angle = 6.2831853f * (float)i / (float)n;
                m.positions.push_back(madrona::math::Vector3 {
                    r * cosf(angle), r * sinf(angle),
                    ring == 0 ? -0.5f * h : 0.5f * h,
                });
            }
        }
        // bottom cap (seen from below), top cap, then the sides
        m.indices.push_back(0);
        for (uint32_t i = n - 1; i >= 1; i--) {
            m.indices.push_back(i);
        }
        m.faceCounts.push_back(n);
        for (uint32_t i = 0; i < n; i++) {
            m.indices.push_back(n + i);
        }
        m.faceCounts.push_back(n);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t j = (i + 1) % n;
            m.indices.push_back(i);
            m.indices.push_back(j);
            m.indices.push_back(n + j);
            m.indices.push_back(n + i);
            m.faceCounts.push_back(4);
        }
        return m;
    }
};

// The collision objects of one simulator, indexed by its object ids (an enum or
// a plain index), over the hulls added so far.
class RigidBodySet {
public:
    explicit RigidBodySet(size_t num_objects)
        : prims_(num_objects), objs_(num_objects)
    {}

    uint32_t addHull(HullSource source)
    {
        hulls_.push_back(std::move(source));
        return (uint32_t)hulls_.size() - 1u;
    }

    template <typename ObjT>
    void hull(ObjT obj, uint32_t hull_idx, float inv_mass,
              madrona::phys::RigidBodyFrictionData friction)
    {
        compound(obj, { hull_idx }, inv_mass, friction);
    }

    // one body of several hulls
    template <typename ObjT>
    void compound(ObjT obj, std::initializer_list<uint32_t> hull_idxs,
                  float inv_mass, madrona::phys::RigidBodyFrictionData friction)
    {
        using madrona::phys::CollisionPrimitive;
        std::vector<madrona::phys::SourceCollisionPrimitive> prims;
        for (uint32_t hull_idx : hull_idxs) {
            madrona::phys::SourceCollisionPrimitive prim {};
            prim.type = CollisionPrimitive::Type::Hull;
            prim.hullInput.hullIDX = hull_idx;
            prims.push_back(prim);
        }
        describe((size_t)obj, std::move(prims), inv_mass, friction);
    }

    template <typename ObjT>
    void sphere(ObjT obj, float radius, float inv_mass,
                madrona::phys::RigidBodyFrictionData friction)
    {
        madrona::phys::SourceCollisionPrimitive prim {};
        prim.type = madrona::phys::CollisionPrimitive::Type::Sphere;
        prim.sphere.radius = radius;
        describe((size_t)obj, { prim }, inv_mass, friction);
    }

    // the static ground plane
    template <typename ObjT>
    void plane(ObjT obj)
    {
        madrona::phys::SourceCollisionPrimitive prim {};
        prim.type = madrona::phys::CollisionPrimitive::Type::Plane;
        describe((size_t)obj, { prim }, 0.f, { 0.5f, 0.5f });
    }

    // Bakes the objects and hands them to a PhysicsLoader for at most
    // max_objects; edit(RigidBodyAssets &) may patch the baked assets before
    // they are loaded.
    template <typename EditFn>
    madrona::phys::ObjectManager *load(const SimCreateArgs &args,
                                       madrona::CountT max_objects, EditFn edit)
    {
        using namespace madrona;
        using namespace madrona::phys;

#ifdef SIM_BACKEND_REF_CPU
        (void)args;
        auto loader = std::make_unique<PhysicsLoader>(ExecMode::CPU, max_objects);
#else
        auto loader = std::make_unique<PhysicsLoader>(ExecMode::CUDA, max_objects,
                                                      args.gpu_id);
#endif

        std::vector<imp::SourceMesh> hull_meshes;
        for (HullSource &source : hulls_) {
            hull_meshes.push_back(source.mesh());
        }

        StackAlloc tmp_alloc;
        RigidBodyAssets rigid_body_assets;
        CountT num_rigid_body_data_bytes;
        void *rigid_body_data = RigidBodyAssets::processRigidBodyAssets(
            Span<const imp::SourceMesh>(hull_meshes.data(),
                                        (CountT)hull_meshes.size()),
            Span<const SourceCollisionObject>(objs_.data(), (CountT)objs_.size()),
            false, tmp_alloc, &rigid_body_assets, &num_rigid_body_data_bytes);

        if (rigid_body_data == nullptr) {
            FATAL("Invalid collision hull input");
        }

        edit(rigid_body_assets);

        loader->loadRigidBodies(rigid_body_assets);
        free(rigid_body_data);

        ObjectManager *mgr = &loader->getObjectManager();
        loaders().push_back(std::move(loader));
        return mgr;
    }

    madrona::phys::ObjectManager *load(const SimCreateArgs &args,
                                       madrona::CountT max_objects)
    {
        return load(args, max_objects, [](madrona::phys::RigidBodyAssets &) {});
    }

private:
    // Loaders stay alive for the life of the process: worlds keep pointing at
    // the ObjectManager they own.
    static std::vector<std::unique_ptr<madrona::phys::PhysicsLoader>> &loaders()
    {
        static std::vector<std::unique_ptr<madrona::phys::PhysicsLoader>> list;
        return list;
    }

    // (an object's Span points into its own vector here: sized up front, the
    // outer vector never moves them)
    void describe(size_t obj,
                  std::vector<madrona::phys::SourceCollisionPrimitive> prims,
                  float inv_mass, madrona::phys::RigidBodyFrictionData friction)
    {
        prims_[obj] = std::move(prims);
        objs_[obj] = madrona::phys::SourceCollisionObject {
            madrona::Span<const madrona::phys::SourceCollisionPrimitive>(
                prims_[obj].data(), (madrona::CountT)prims_[obj].size()),
            inv_mass,
            friction,
        };
    }

    std::vector<HullSource> hulls_;
    std::vector<std::vector<madrona::phys::SourceCollisionPrimitive>> prims_;
    std::vector<madrona::phys::SourceCollisionObject> objs_;
};

// edit for load(): agents turn about z only (infinite inertia about x and y)
template <typename ObjT>
auto turnAboutZOnly(ObjT obj)
{
    return [obj](madrona::phys::RigidBodyAssets &assets) {
        assets.metadatas[(size_t)obj].mass.invInertiaTensor.x = 0.f;
        assets.metadatas[(size_t)obj].mass.invInertiaTensor.y = 0.f;
    };
}

}
